"""Letter-pair counts under hits on the device (pfmscan_site_joint_*): the kernel against the plain loop of
tests/site_joint_rules.py, tables equal as integers, in both entry-point forms; rejections; the command line on FASTA inputs
against the same command on the rules engine, byte for byte."""
import os

import numpy as np
import pytest

import site_joint_rules as jr
from pairsum_helpers import streams

pytestmark = pytest.mark.gpu

COLS = 64


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


def test_constants():
    from rnascan_amd import _lib
    assert _lib.SITE_JOINT_COLS == COLS and _lib.ABI_VERSION >= 19


def pair_stream(rng, lengths, foreign=0.05):
    from rnascan_amd import pack
    s1, s2 = streams(rng, lengths, foreign)
    return pack.Stream(s1.codes, None, s1.offsets, s1.lengths, codes2=s2.codes)


def windows(st, m):
    return np.flatnonzero(st.window_mask(m)).astype(np.int64)


def motif_major(pos, motif):
    order = np.lexsort((pos, motif))
    return pos[order], motif[order]


def dev_form(ctx, st, pos, motif, n_motifs, m, flank, first=True, second=True, n_pos=None, tables=None):
    """pfmscan_site_joint_dev on torch buffers (the list as given: motif-major) -> uint64 [n_motifs][W][8][8]"""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)            # noqa: E731
    codes, codes2 = (up(st.codes) if first else None), (up(st.codes2) if second else None)
    d_pos = up(np.asarray(pos, dtype=np.int64))
    d_mo = None if motif is None else up(np.asarray(motif, dtype=np.int32))
    offsets, lengths = tables if tables is not None else (st.offsets, st.lengths)
    off, ln = up(np.asarray(offsets, dtype=np.int64)), up(np.asarray(lengths, dtype=np.int64))
    joint = torch.full((max(n_motifs, 1), m + 2 * flank, 8, 8), -1, dtype=torch.int64, device=dev)     # it zeroes the table itself
    torch.cuda.synchronize()
    ctx.site_joint_dev(codes, codes2, len(st.codes) if n_pos is None else n_pos, d_pos, d_mo, len(pos), off, ln, len(offsets),
                       n_motifs, m, flank, joint)
    ctx.synchronize()
    return joint.cpu().numpy().view(np.uint64)[:n_motifs]


def check(engine, st, pos, motif, n_motifs, m, flank, first=True, second=True, want=None):
    """both forms against the rule (computed once per case); ``pos`` / ``motif`` in (position, motif) order"""
    if want is None:
        want = jr.site_joint(st.codes if first else None, st.codes2 if second else None, pos, motif, n_motifs, st.offsets,
                             st.lengths, m, flank)
    staged = engine.site_joint(st, pos, motif, n_motifs, m, flank, first=first, second=second)
    assert staged.dtype == np.uint64 and staged.shape == want.shape and np.array_equal(staged, want)
    p, k = (pos, None) if motif is None else motif_major(pos, motif)
    dev = dev_form(engine.ctx, st, p, k, n_motifs, m, flank, first, second)
    assert np.array_equal(dev, want)
    return want


# ---- widths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,flank", [(1, 0), (COLS - 1, 0), (COLS - 2, 1), (COLS - 1, 1), (5, COLS - 2), (1, COLS)],
                         ids=["W1", "Wcols-1", "Wcols", "Wcols+1", "W2cols+1", "W2cols+1-flanks"])
def test_widths_around_the_column_tile(engine, m, flank):
    rng = np.random.default_rng(100 * m + flank)
    st = pair_stream(rng, [m, 1, m + 1, 200, max(m - 1, 0), 2 * m + 3, 90, m, 1, 150])
    pos = windows(st, m)
    assert pos[0] == 0 and pos[-1] == st.offsets[-1] + st.lengths[-1] - m           # the first and the last window of the stream
    pos = np.union1d(pos[rng.random(pos.size) < 0.25], pos[[0, -1]])
    motif = rng.integers(0, 3, size=pos.size).astype(np.int32)
    want = check(engine, st, pos, motif, 3, m, flank)
    W = m + 2 * flank
    assert W in (1, COLS - 1, COLS, COLS + 1, 2 * COLS + 1) and want.sum() > 0
    if flank:
        assert want.sum(axis=(0, 2, 3)).min() < pos.size                           # flanks hang over record ends


def test_widest_table_on_a_handful_of_hits(engine):
    rng = np.random.default_rng(4096)
    m, flank = 64, 2016
    st = pair_stream(rng, [64, 5000, 65, 300])                                   # every record but one shorter than W
    pos = np.asarray([0, st.offsets[1] + 7, st.offsets[1] + 2500, st.offsets[1] + 5000 - 64, st.offsets[2] + 1, st.offsets[3] + 236])
    motif = np.asarray([1, 0, 1, 1, 0, 1], dtype=np.int32)
    want = check(engine, st, pos, motif, 2, m, flank)
    from rnascan_amd import sites
    assert want.shape[1] == 4096 and want[1].sum(axis=(1, 2)).max() == 4
    assert np.array_equal(want.sum(axis=(0, 2, 3)).astype(np.int64), sites.coverage(st, pos, m, flank))


# ---- hit counts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hits", [0, 1, 63, 64, 65])
def test_hit_counts_around_a_wave(engine, n_hits):
    rng = np.random.default_rng(n_hits)
    st = pair_stream(rng, [40, 12, 300, 13])
    pos = np.sort(rng.choice(windows(st, 12), size=n_hits, replace=False))
    check(engine, st, pos, None, 1, 12, 3)
    check(engine, st, pos, rng.integers(0, 2, size=n_hits).astype(np.int32), 2, 12, 3)


def test_several_slices_and_a_motif_change_inside_one(engine, monkeypatch):
    rng = np.random.default_rng(7)
    st = pair_stream(rng, [int(x) for x in rng.integers(20, 400, size=30)])
    pos = windows(st, 9)
    pos = pos[rng.random(pos.size) < 0.4]
    # motif 2 has no hit; the change 0 -> 1 falls inside a wave's 64 hits (not on a multiple of 64) and inside a slice
    motif = (np.arange(pos.size) % 5 == 0).astype(np.int32) * 3
    motif[rng.random(pos.size) < 0.5] = 1
    n0 = int((motif == 0).sum())
    assert pos.size > 1500 and n0 % 64 not in (0, 63) and not (motif == 2).any()
    want = check(engine, st, pos, motif, 4, 9, 2)
    assert not want[2].any() and want[0].any() and want[3].any()
    for slice_ in ("1", "64", "100", "256", "1000"):                             # the table does not depend on the slice
        monkeypatch.setenv("PFMSCAN_SITE_JOINT_SLICE", slice_)
        check(engine, st, pos, motif, 4, 9, 2, want=want)


def test_one_cell_hit_by_every_lane(engine):
    """one record of one letter pair, densely hit: every lane adds to the same LDS cell of a column"""
    from rnascan_amd import pack
    n, m = 200000, 2
    st = pack.Stream(np.append(np.full(n + m - 1, 2, dtype=np.uint8), np.uint8(7)), None, np.asarray([0]), np.asarray([n + m - 1]),
                     codes2=np.append(np.full(n + m - 1, 5 | 8, dtype=np.uint8), np.uint8(7)))
    pos = np.arange(n, dtype=np.int64)
    want = check(engine, st, pos, None, 1, m, 0)
    assert want[0, :, 2, 5].tolist() == [n, n] and want.sum() == 2 * n


def test_257_motifs(engine):
    rng = np.random.default_rng(257)
    st = pair_stream(rng, [int(x) for x in rng.integers(10, 120, size=20)])
    pos = windows(st, 6)
    motif = rng.integers(0, 257, size=pos.size).astype(np.int32)
    motif[motif == 100] = 101
    want = check(engine, st, pos, motif, 257, 6, 1)
    assert not want[100].any() and want[256].any() and want[0].any()


# ---- streams --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,second", [(True, False), (False, True), (True, True)], ids=["codes", "codes2", "both"])
def test_either_stream_alone(engine, first, second):
    rng = np.random.default_rng(3)
    st = pair_stream(rng, [50, 7, 8, 120, 33], foreign=0.1)
    assert (st.codes2 & 8).any() and (st.codes[:50] == 7).any() and (st.codes2[:50] == 7).any()      # case bits; code 7 inside records
    pos = windows(st, 7)
    motif = rng.integers(0, 2, size=pos.size).astype(np.int32)
    want = check(engine, st, pos, motif, 2, 7, 4, first, second)
    assert want[:, :, 7 if first else 0, :].any() and want[:, :, :, 7 if second else 0].any()
    if not first:
        assert not want[:, :, 1:, :].any()
    if not second:
        assert not want[:, :, :, 1:].any()
    if second:                                                                   # a lower-case letter counts under its letter
        upper = type(st)(st.codes, None, st.offsets, st.lengths, codes2=st.codes2 & 7)
        assert np.array_equal(engine.site_joint(upper, pos, motif, 2, 7, 4, first=first, second=True), want)


def test_two_runs_give_the_same_bytes(engine):
    rng = np.random.default_rng(21)
    st = pair_stream(rng, [int(x) for x in rng.integers(30, 300, size=40)])
    pos = windows(st, 11)
    motif = rng.integers(0, 5, size=pos.size).astype(np.int32)
    a = engine.site_joint(st, pos, motif, 5, 11, 6)
    b = engine.site_joint(st, pos, motif, 5, 11, 6)
    p, k = motif_major(pos, motif)
    c, d = dev_form(engine.ctx, st, p, k, 5, 11, 6), dev_form(engine.ctx, st, p, k, 5, 11, 6)
    assert a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes()


# ---- past 2^31 ------------------------------------------------------------------------------------------------------------
def test_positions_beyond_2_31(engine):
    """both streams made on the device and longer than 2^31 positions; the hits lie in the last record, whose positions no
    32-bit integer holds; the expectation comes from the rule on that record alone"""
    import torch
    if torch.cuda.mem_get_info()[0] < 8e9:
        pytest.skip("needs 8 GB of free HBM")
    dev = torch.device("cuda", 0)
    m, flank, tail = 12, 5, 700
    n_pos = (1 << 31) + 5000
    g = torch.Generator(device=dev)
    g.manual_seed(6)
    codes = torch.randint(0, 4, (n_pos,), device=dev, generator=g, dtype=torch.uint8)
    codes2 = torch.randint(0, 15, (n_pos,), device=dev, generator=g, dtype=torch.uint8)          # letters, case bits and 7s
    first = n_pos - tail - 1                                                     # the last record: positions [first, first + tail)
    assert first > (1 << 31)
    offsets, lengths = np.asarray([0, first], dtype=np.int64), np.asarray([first - 1, tail], dtype=np.int64)
    local1, local2 = codes[first:first + tail + 1].cpu().numpy(), codes2[first:first + tail + 1].cpu().numpy()
    start = np.asarray([0, 1, 2, 3, 4, 9, 300, 301, tail - m - 1, tail - m], dtype=np.int64)
    motif = np.asarray([0, 0, 0, 1, 1, 1, 1, 2, 2, 2], dtype=np.int32)
    want = jr.site_joint(local1, local2, start, motif, 3, [0], [tail], m, flank)
    up = lambda a: torch.from_numpy(a).to(dev)                                   # noqa: E731
    d_pos, d_mo, off, ln = up(start + first), up(motif), up(offsets), up(lengths)
    joint = torch.full((3, m + 2 * flank, 8, 8), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    engine.ctx.site_joint_dev(codes, codes2, n_pos, d_pos, d_mo, start.size, off, ln, 2, 3, m, flank, joint)
    engine.ctx.synchronize()
    assert np.array_equal(joint.cpu().numpy().view(np.uint64), want) and want.sum() > 0
    del codes, codes2
    torch.cuda.empty_cache()


# ---- broken input ---------------------------------------------------------------------------------------------------------
def test_broken_input_is_refused_and_the_context_stays_usable(engine):
    rng = np.random.default_rng(13)
    st = pair_stream(rng, [30, 10, 25])
    m = 8
    good = windows(st, m)
    motif = np.sort(rng.integers(0, 3, size=good.size)).astype(np.int32)
    want = check(engine, st, good, motif, 3, m, 2)
    n_pos = len(st.codes)
    over = good.copy()
    over[5] = st.offsets[0] + 30 - m + 1                                         # the window runs over its record's end
    beyond = good.copy()
    beyond[-1] = n_pos
    negative = good.copy()
    negative[0] = -1
    no_motif = motif.copy()
    no_motif[-1] = 3
    minus = motif.copy()
    minus[0] = -1
    descending = motif.copy()
    descending[4], descending[5] = 1, 0
    assert descending[3] == 0 and descending[6] == 0
    for pos, mo in ((over, motif), (beyond, motif), (negative, motif), (good, no_motif), (good, minus), (good, descending)):
        with pytest.raises(ValueError):
            dev_form(engine.ctx, st, pos, mo, 3, m, 2)
        p, k = motif_major(good, motif)
        assert np.array_equal(dev_form(engine.ctx, st, p, k, 3, m, 2), want)    # the next valid call on the same context
    for pos, mo in ((over, motif), (beyond, motif), (good, no_motif)):             # the staged form: the same verdicts
        with pytest.raises(ValueError):
            engine.site_joint(st, pos, mo, 3, m, 2)
        assert np.array_equal(engine.site_joint(st, good, motif, 3, m, 2), want)
    # a record table whose record lies outside the stream: nothing is read there
    with pytest.raises(ValueError):
        dev_form(engine.ctx, st, good, motif, 3, m, 2, tables=(st.offsets, np.asarray([30, 10, 1 << 40])))
    with pytest.raises(ValueError):
        dev_form(engine.ctx, st, good[:3], None, 0, m, 2)                        # hits but no motif
    with pytest.raises(ValueError):
        engine.ctx.site_joint_staged(good, motif, 3, st.offsets, st.lengths, 4000, 100)          # W > PFMSCAN_MAX_WIDTH
    assert np.array_equal(engine.site_joint(st, good, motif, 3, m, 2), want)


# ---- the command ----------------------------------------------------------------------------------------------------------
SUFFIXES = ("struct", "seq", "joint", "counts")


def _files(prefix):
    out = {}
    for suffix in SUFFIXES:
        path = "%s.%s.txt" % (prefix, suffix)
        if os.path.exists(path):
            out[suffix] = open(path, "rb").read()
    return out


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from sites_lib_helpers import write_library
    tmp = tmp_path_factory.mktemp("site_joint_gpu")
    fa, sfa, _ = jr.write_letter_inputs(tmp, n=60, seed=9)
    lib_seq, lib_struct, _ = write_library(tmp)
    return tmp, fa, sfa, lib_seq, lib_struct


def _both(engine, tmp, name, argv):
    from rnascan_amd import sites
    rc_rules = sites.main(argv[:1] + [str(tmp / (name + "_rules"))] + argv[1:], engine=jr.RulesEngine())
    rc = sites.main(argv[:1] + [str(tmp / (name + "_gpu"))] + argv[1:], engine=engine)
    want, got = _files(tmp / (name + "_rules")), _files(tmp / (name + "_gpu"))
    assert rc == rc_rules == 0 and sorted(got) == sorted(want) and len(want) >= 2
    for suffix in want:
        assert got[suffix] == want[suffix], suffix
    return want


@pytest.mark.parametrize("form", ["seq", "struct", "pair", "pair-sum", "pair-sum-inf", "learn"])
def test_command_equals_the_rules_engine_byte_for_byte(engine, inputs, form):
    from sites_lib_helpers import SEQ_PFM, STRUCT_PFM
    tmp, fa, sfa, _, _ = inputs
    argv = {"seq": ["-p", SEQ_PFM, "-m", "4", fa],
            "struct": ["-q", STRUCT_PFM, "-C", "0.05", "-m", "2", sfa],
            "pair": ["-p", SEQ_PFM, "-q", STRUCT_PFM, "-C", "0.05", "-m", "-8", fa, sfa],
            "pair-sum": ["-p", SEQ_PFM, "-q", STRUCT_PFM, "-C", "0.05", "-m", "-30", "--min-seqstruct", "-20", fa, sfa],
            "pair-sum-inf": ["-p", SEQ_PFM, "-q", STRUCT_PFM, "-C", "0.05", "-m", " -inf", "--min-seqstruct", "-20", fa, sfa],
            "learn": ["-p", SEQ_PFM, "-m", "4", fa, sfa]}[form]
    want = _both(engine, tmp, form, ["-o", "--flank", "3"] + argv)
    assert sorted(want) == sorted({"seq": ["counts", "seq"], "struct": ["counts", "struct"]}.get(form, list(SUFFIXES)))
    assert want["counts"].count(b"\n") == 1 + 18 + 6


@pytest.mark.parametrize("form", ["seq", "struct", "pair", "pair-sum", "learn"])
def test_all_motifs_equals_the_rules_engine_byte_for_byte(engine, inputs, form):
    tmp, fa, sfa, lib_seq, lib_struct = inputs
    argv = {"seq": ["-p", lib_seq, "-m", "4", fa],
            "struct": ["-q", lib_struct, "-C", "0.05", "-m", "2", sfa],
            "pair": ["-p", lib_seq, "-q", lib_struct, "-C", "0.05", "-m", "-8", fa, sfa],
            "pair-sum": ["-p", lib_seq, "-q", lib_struct, "-C", "0.05", "-m", "-30", "--min-seqstruct", "-20", fa, sfa],
            "learn": ["-p", lib_seq, "-m", "4", fa, sfa]}[form]
    want = _both(engine, tmp, "all_" + form, ["-o", "--all-motifs", "--flank", "2"] + argv)
    assert want["counts"].startswith(b"Motif\tPO\tSites\tCoverage\t") and want["counts"].count(b"\n") == 1 + 2 * (18 + 4) + 2 * (12 + 4)


def test_dot_bracket_structure_fasta(engine, tmp_path):
    from background_helpers import write_fasta
    from dotbracket_rules import annotate, random_structure
    from sites_lib_helpers import SEQ_PFM, STRUCT_PFM
    rng = np.random.default_rng(11)
    seqs = [("d%02d" % i, "".join(rng.choice(list("ACGU"), size=int(rng.integers(30, 200))))) for i in range(12)]
    db = [(rid, random_structure(rng, len(s))) for rid, s in seqs]
    fa, dbfa, sfa = str(tmp_path / "seqs.fa"), str(tmp_path / "db.fa"), str(tmp_path / "letters.fa")
    write_fasta(fa, seqs)
    write_fasta(dbfa, db)
    write_fasta(sfa, [(rid, annotate(s)) for rid, s in db])
    tail = ["-p", SEQ_PFM, "-q", STRUCT_PFM, "-C", "0.05", "-m", "-16", "--flank", "2", fa]
    want = _both(engine, tmp_path, "db", ["-o"] + tail + [dbfa])
    assert len(want) == 4 and _both(engine, tmp_path, "letters", ["-o"] + tail + [sfa]) == want


def test_command_on_two_ranks_of_the_one_gpu_writes_the_same_files(inputs, tmp_path):
    """`--gpus 2` as tests/test_gpu_launch.py rehearses it: two ranks share device 0"""
    import subprocess
    import sys
    from conftest import REPO
    from sites_lib_helpers import SEQ_PFM, STRUCT_PFM
    _, fa, sfa, _, _ = inputs
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["PYTHONPATH"] = os.pathsep.join([REPO] + [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    tail = ["-p", SEQ_PFM, "-q", STRUCT_PFM, "-C", "0.05", "-m", "-30", "--min-seqstruct", "-20", "--flank", "3", fa, sfa]
    cmd = [sys.executable, "-m", "rnascan_amd.sites"]
    one = subprocess.run(cmd + ["-o", str(tmp_path / "one")] + tail, env=env, capture_output=True, text=True, timeout=280)
    assert one.returncode == 0, one.stderr[-3000:]
    two = subprocess.run(cmd + ["-o", str(tmp_path / "two"), "--gpus", "2"] + tail, env=dict(env, RNASCAN_ONE_DEVICE="1"),
                         capture_output=True, text=True, timeout=280)
    assert two.returncode == 0, two.stderr[-3000:]
    a, b = _files(tmp_path / "one"), _files(tmp_path / "two")
    assert sorted(a) == sorted(SUFFIXES) and a == b and a["joint"].count(b"\n") == 1 + 18 + 6
