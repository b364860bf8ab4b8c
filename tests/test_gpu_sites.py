"""Site profiles on the device (pfmscan_site_sums_*): group sums and counts against the numpy restatement of their groups
and order of additions (tests/sites_rules.py), BIT FOR BIT -- ``sums.view(uint64)`` and ``counts`` -- in every entry-point
form; rejections; broken tables; the command line against the same command on the restated rules."""
import os

import numpy as np
import pytest

import sites_rules as rules
from background_helpers import random_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make_stream(rng, lengths, dtype, scale=True):
    from rnascan_amd import pack
    profs, codes = [], []
    for L in lengths:
        p = random_rows(rng, L) * (rng.choice([1.0, 1e-7, 1e4]) if scale else 1.0)
        profs.append(p.astype(dtype))
        codes.append(rng.choice(np.arange(8, dtype=np.uint8), size=L, p=[.22, .22, .22, .22, .03, .03, .03, .03]))
    return pack.pack(code_arrays=codes, profiles=profs, profile_dtype=dtype)


def windows(st, m):
    return np.flatnonzero(st.window_mask(m)).astype(np.int64)


def dev_form(ctx, st, pos, m, flank, grp_first=None, grp_rec=None, stream=None):
    """pfmscan_site_sums_dev on torch buffers -> (sums, counts)"""
    import torch
    dev = torch.device("cuda", 0)
    if grp_first is None:
        grp_first, grp_rec = rules.groups(pos, st.offsets, st.lengths, m)
    W = m + 2 * flank
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)            # noqa: E731
    prof, codes, d_pos = up(st.profile), up(st.codes), up(np.asarray(pos, dtype=np.int64))
    gf, gr, off, ln = up(grp_first), up(grp_rec), up(st.offsets), up(st.lengths)
    sums = torch.full((max(len(grp_rec), 1), W, 7), -1.0, dtype=torch.float64, device=dev)
    counts = torch.full((max(len(grp_rec), 1), W, 8), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.site_sums_dev(codes.data_ptr(), prof.data_ptr(), st.profile.dtype, st.profile.shape[0], d_pos.data_ptr(), len(pos),
                      gf.data_ptr(), gr.data_ptr() if len(grp_rec) else 0, len(grp_rec), off.data_ptr(), ln.data_ptr(),
                      len(st.offsets), m, flank, sums.data_ptr(), counts.data_ptr(), stream=stream)
    ctx.synchronize()
    torch.cuda.synchronize()
    return sums.cpu().numpy()[:len(grp_rec)], counts.cpu().numpy().view(np.uint32)[:len(grp_rec)]


def check(engine, st, pos, m, flank, chunk="3000"):
    """every form against the rules; returns the expected (grp_rec, sums, counts)"""
    ctx = engine.ctx
    want = rules.site_sums(st.profile, st.codes, pos, st.offsets, st.lengths, m, flank)
    forms = {"host": ctx.site_sums_host(st.codes, st.profile, pos, st.offsets, st.lengths, m, flank)}
    os.environ["PFMSCAN_SITES_CHUNK"] = chunk
    try:
        forms["chunked"] = ctx.site_sums_host(st.codes, st.profile, pos, st.offsets, st.lengths, m, flank)
    finally:
        del os.environ["PFMSCAN_SITES_CHUNK"]
    ctx.stage(st.codes, st.profile)
    forms["staged"] = ctx.site_sums_staged(pos, st.offsets, st.lengths, m, flank)
    forms["dev"] = (want[0],) + dev_form(ctx, st, pos, m, flank)
    for name, got in forms.items():
        assert np.array_equal(got[0], want[0]), name
        assert got[1].shape == want[1].shape and got[2].shape == want[2].shape, name
        assert np.array_equal(bits(got[1]), bits(want[1])), (name, m, flank, np.argwhere(bits(got[1]) != bits(want[1]))[:5])
        assert np.array_equal(got[2], want[2]), (name, m, flank, np.argwhere(got[2] != want[2])[:5])
    # coverage from positions and record bounds alone == the counts' row sums
    assert np.array_equal(want[2].astype(np.int64).sum(axis=(0, 2)), rules.coverage(pos, st.offsets, st.lengths, m, flank))
    return want


# ---- bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m", [1, 9, 10, 12, 18, 19, 64, 65, 600])
def test_sums_and_counts_equal_the_restatement_bit_for_bit(engine, m, dtype):
    """cell counts 7, 63 / 70, 84, 126 / 133 and 448 straddle the 64-lane chunks; 65 and 600 take the multi-chunk walk.
    Records of length m, m + 1 and shorter than W; hits at a record's first window and at the stream's last window; odd
    record lengths leave the rows off 16-byte alignment."""
    rng = np.random.default_rng(100 + m)
    lengths = [m, m + 1, m + 2, 3, m + 37, 2 * m + 5, m, m + 201, 0, m + 3 * m // 2 + 1, m + 11]
    st = make_stream(rng, lengths, dtype)
    assert len({int(o) * 7 * np.dtype(dtype).itemsize % 16 for o in st.offsets}) > 1
    win = windows(st, m)
    keep = rng.random(win.size) < 0.3
    keep[0] = keep[-1] = True
    first = np.searchsorted(win, st.offsets[np.asarray(lengths) >= m])
    keep[first] = True                                               # every record's first window
    pos = win[keep]
    assert pos[-1] + m == st.offsets[-1] + st.lengths[-1]             # the stream's last window
    for flank in (0, 3, m, 200):
        if m + 2 * flank <= 4096:
            check(engine, st, pos, m, flank, chunk=str(2 * m + 40))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_groups_of_every_size_dense_hits(engine, dtype):
    """records with exactly 1, 2, 3, 4, 5, 63, 64, 65, 4096, 4097 and 8195 windows, every window a hit (the dense record
    of 8.2k rows is the largest shape): groups of those sizes and the remainders 1 and 3 behind full groups"""
    rng = np.random.default_rng(7)
    m = 12
    sizes = [1, 2, 3, 4, 5, 63, 64, 65, 4096, 4097, 8195]
    st = make_stream(rng, [n + m - 1 for n in sizes], dtype)
    pos = windows(st, m)
    grp_rec, _, _ = check(engine, st, pos, m, 0, chunk="5000")
    got = sorted(np.diff(rules.groups(pos, st.offsets, st.lengths, m)[0]).tolist())
    assert got == sorted([1, 2, 3, 4, 5, 63, 64, 65, 4096, 4096, 1, 4096, 4096, 3])
    assert grp_rec.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 10, 10, 10]
    check(engine, st, pos, m, 3, chunk="9000")


def test_sparse_hits_and_no_hits(engine):
    rng = np.random.default_rng(8)
    st = make_stream(rng, rng.integers(0, 300, size=400).tolist(), np.float64)
    win = windows(st, 10)
    check(engine, st, win[rng.random(win.size) < 0.002], 10, 5, chunk="2000")
    check(engine, st, win[:0], 10, 5)
    check(engine, st, win[-1:], 10, 0)


def test_one_hit_gives_the_rows_under_it(engine):
    st = make_stream(np.random.default_rng(9), [50, 40], np.float64)
    pos = np.asarray([int(st.offsets[1]) + 7], dtype=np.int64)
    _, sums, counts = engine.site_sums(st, pos, 9)
    assert np.array_equal(bits(sums[0]), bits(st.profile[pos[0]:pos[0] + 9]))
    assert np.array_equal(np.argmax(counts[0], axis=1), np.minimum(st.codes[pos[0]:pos[0] + 9], 7))


# ---- rejections --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf, -1e-300])
def test_a_bad_cell_under_a_hit_is_rejected_with_the_earliest_cell(engine, value):
    rng = np.random.default_rng(10)
    st = make_stream(rng, [40, 30, 60], np.float64, scale=False)
    m, flank = 8, 4
    pos = np.asarray([st.offsets[0] + 5, st.offsets[1] + 0, st.offsets[1] + 22, st.offsets[2] + 30], dtype=np.int64)
    # under no hit; in a separator row and in the neighbour's first rows, which the flank of the hit at the record end skips
    for row, col in ((int(st.offsets[0]) + 30, 2), (int(st.offsets[1]) + 30, 0), (int(st.offsets[2]) + 1, 6)):
        st.profile[row, col] = value
    assert rules.first_bad(st.profile, pos, st.offsets, st.lengths, m, flank) == -1
    check(engine, st, pos, m, flank)
    # under a flank column and under the window: the earliest touched cell is named by every form
    st.profile[int(st.offsets[2]) + 33, 1] = value
    st.profile[int(st.offsets[1]) + 19, 5] = value                    # the left flank of the hit at offsets[1] + 22
    want = rules.first_bad(st.profile, pos, st.offsets, st.lengths, m, flank)
    assert want == (int(st.offsets[1]) + 19) * 7 + 5
    ctx = engine.ctx
    calls = [lambda: ctx.site_sums_host(st.codes, st.profile, pos, st.offsets, st.lengths, m, flank),
             lambda: dev_form(ctx, st, pos, m, flank),
             lambda: (ctx.stage(st.codes, st.profile), ctx.site_sums_staged(pos, st.offsets, st.lengths, m, flank))]
    os.environ["PFMSCAN_SITES_CHUNK"] = "45"
    try:
        for call in calls:
            with pytest.raises(ValueError) as e:
                call()
            assert e.value.element == want
    finally:
        del os.environ["PFMSCAN_SITES_CHUNK"]
    # without the flank only the cell under the window of the last hit is touched
    with pytest.raises(ValueError) as e:
        engine.site_sums(st, pos, m, 0)
    assert e.value.element == (int(st.offsets[2]) + 33) * 7 + 1


def test_broken_tables_are_refused_by_the_device_check(engine):
    """k_site_check decides: PFMSCAN_E_BADARG (ValueError without ``element``); the sums kernel clamps every index it takes
    from the tables, so nothing is read outside the buffers"""
    rng = np.random.default_rng(11)
    m = 6
    st = make_stream(rng, [30, 5000, 20], np.float64)
    pos = windows(st, m)
    gf, gr = rules.groups(pos, st.offsets, st.lengths, m)
    assert gf.size == 5                                              # 25 | 4096 + 899 | 15
    dev_form(engine.ctx, st, pos, m, 2, gf, gr)                      # the table as it should be

    def refused(pos=pos, gf=gf, gr=gr, off=st.offsets, ln=st.lengths):
        from rnascan_amd import pack
        broken = pack.Stream(st.codes, st.profile, off, ln)
        with pytest.raises(ValueError) as e:
            dev_form(engine.ctx, broken, pos, m, 2, gf, gr)
        assert getattr(e.value, "element", None) is None

    refused(gf=np.asarray([0, 25, 20, 5020, 5035]))                  # not monotone
    refused(gf=np.asarray([0, 25, 4121, 5020, 5030]))                # does not end at n_hits
    refused(gf=np.asarray([1, 25, 4121, 5020, 5035]))                # does not start at the first hit
    refused(gf=np.asarray([0, 25, 4122, 5020, 5035]))                # a group of 4097
    refused(gf=np.asarray([0, 26, 4121, 5020, 5035]))                # a hit in the group of another record
    refused(gr=np.asarray([0, 1, 1, 3]))                             # a record that does not exist
    refused(gr=np.asarray([0, 1, 1, -1]))
    refused(gr=np.asarray([0, 1, 0, 2]))
    swapped = pos.copy()
    swapped[[100, 101]] = swapped[[101, 100]]
    refused(pos=swapped)                                             # hits that descend
    same = pos.copy()
    same[200] = same[199]
    refused(pos=same)
    late = pos.copy()
    late[24] += 1
    refused(pos=late)                                                # a window across the separator
    wild = pos.copy()
    wild[-1] = np.iinfo(np.int64).max - 2
    refused(pos=wild)
    wild[-1] = np.iinfo(np.int64).min
    refused(pos=wild)
    refused(ln=np.asarray([30, 5000, 22]))                           # a record that leaves the stream
    refused(off=np.asarray([0, 31, 1 << 40]))
    refused(off=np.asarray([-1, 31, 5032]))


def test_dev_form_on_a_callers_stream_with_device_made_inputs(engine):
    """rows, hits and tables made on the device on a non-default stream, the sums enqueued behind them on that stream"""
    import torch
    from rnascan_amd import pack
    ctx = engine.ctx
    dev = torch.device("cuda", 0)
    m, flank, L, R = 19, 3, 700, 9
    W = m + 2 * flank
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        g = torch.Generator(device=dev)
        g.manual_seed(5)
        n_pos = R * (L + 1)
        prof = torch.randint(0, 1024, (n_pos, 7), device=dev, generator=g).to(torch.float32) / 1024.0
        codes = torch.randint(0, 8, (n_pos,), device=dev, generator=g).to(torch.uint8)
        off = torch.arange(R, device=dev, dtype=torch.int64) * (L + 1)
        ln = torch.full((R,), L, device=dev, dtype=torch.int64)
        start = torch.arange(0, L - m + 1, 3, device=dev, dtype=torch.int64)
        pos = (off[:, None] + start[None, :]).reshape(-1).contiguous()
        per = start.numel()
        gf = torch.arange(R + 1, device=dev, dtype=torch.int64) * per
        gr = torch.arange(R, device=dev, dtype=torch.int64)
        sums = torch.empty((R, W, 7), dtype=torch.float64, device=dev)
        counts = torch.empty((R, W, 8), dtype=torch.int32, device=dev)
        ctx.site_sums_dev(codes.data_ptr(), prof.data_ptr(), np.float32, n_pos, pos.data_ptr(), pos.numel(), gf.data_ptr(),
                          gr.data_ptr(), R, off.data_ptr(), ln.data_ptr(), R, m, flank, sums.data_ptr(), counts.data_ptr(),
                          stream=s.cuda_stream)
        doubled = sums * 2                                            # enqueued behind the sums on the same stream
    s.synchronize()
    st = pack.Stream(codes.cpu().numpy(), prof.cpu().numpy(), off.cpu().numpy(), ln.cpu().numpy())
    grp_rec, want_s, want_c = rules.site_sums(st.profile, st.codes, pos.cpu().numpy(), st.offsets, st.lengths, m, flank)
    assert grp_rec.tolist() == list(range(R))
    assert np.array_equal(bits(sums.cpu().numpy()), bits(want_s))
    assert np.array_equal(bits(doubled.cpu().numpy()), bits(want_s * 2))
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), want_c)


def test_host_form_pieces_upload_modes_and_the_staged_stream(engine, tmp_path, monkeypatch):
    """a mapped float32 stream of 45 MB (the staged uploader takes part when forced): the same bits in both upload modes,
    for >= 3 pieces and for one, with a record longer than the chunk as a piece of its own; the stream staged before is
    still scannable afterwards"""
    from rnascan_amd import pack
    ctx = engine.ctx
    rng = np.random.default_rng(12)
    lengths = rng.integers(2000, 4000, size=540)
    lengths[17] = 90000
    n_pos = int(lengths.sum() + lengths.size)
    path = str(tmp_path / "rows.f32")
    rows = np.zeros((n_pos, 7), dtype=np.float32)
    offsets = np.zeros(lengths.size, dtype=np.int64)
    offsets[1:] = np.cumsum(lengths[:-1] + 1)
    for o, L in zip(offsets, lengths):
        rows[o:o + L] = random_rows(rng, 64)[rng.integers(0, 64, size=L)]
    rows.tofile(path)
    mapped = np.memmap(path, dtype=np.float32, mode="r", shape=(n_pos, 7))
    codes = rng.integers(0, 4, size=n_pos).astype(np.uint8)
    st = pack.Stream(codes, mapped, offsets, lengths)
    m, flank = 12, 20
    win = windows(st, m)
    keep = rng.random(win.size) < 3e-4
    keep[np.searchsorted(win, offsets[17]):np.searchsorted(win, offsets[17]) + 5000:2] = True     # dense in the long record
    pos = win[keep]
    want = rules.site_sums(rows, codes, pos, offsets, lengths, m, flank)
    # another stream is staged and scanned before and after
    small = make_stream(rng, [300, 200], np.float64, scale=False)
    P = np.log2(random_rows(rng, 9) * 7 + 0.01)
    before = engine.hits(small, None, P, -np.inf, -1000.0)
    seen = []
    for upload in ("0", "1"):
        for chunk in ("70000", None):
            monkeypatch.setenv("PFMSCAN_UPLOAD", upload)
            if chunk:
                monkeypatch.setenv("PFMSCAN_SITES_CHUNK", chunk)
            else:
                monkeypatch.delenv("PFMSCAN_SITES_CHUNK", raising=False)
            seen.append(engine.site_sums(st, pos, m, flank))
    monkeypatch.delenv("PFMSCAN_UPLOAD")
    for got in seen:
        assert np.array_equal(got[0], want[0])
        assert np.array_equal(bits(got[1]), bits(want[1]))
        assert np.array_equal(got[2], want[2])
    assert n_pos > 3 * 70000 and lengths[17] > 70000
    after = ctx.hits_staged(engine._motif(None, P), -np.inf, -1000.0)
    assert before[0].size > 0 and np.array_equal(before[0], after[0]) and np.array_equal(bits(before[2]), bits(after[2]))


# ---- the command, end to end, against the same command on the restated rules ------------------------------------------------
def _command(argv, engine, prefix):
    from rnascan_amd import sites
    rc = sites.main(["-o", prefix] + list(argv), engine=engine)
    out = {}
    for suffix in ("struct", "seq", "counts"):
        path = "%s.%s.txt" % (prefix, suffix)
        if os.path.exists(path):
            out[suffix] = open(path, "rb").read()
    return rc, out


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from sites_helpers import write_inputs
    return write_inputs(tmp_path_factory.mktemp("sites"), n=60)


CASES = {"p_only": ["-p", "SEQ", "-m", "4"],
         "p_only_flank": ["-p", "SEQ", "-m", "4", "--flank", "9"],
         "q_only": ["-q", "STRUCT", "-C", "0.05", "-m", "-14"],
         "q_only_flank_float32": ["-q", "STRUCT", "-C", "0.05", "-m", "-14", "--flank", "30", "--profile-dtype", "float32"],
         "both": ["-p", "SEQ", "-q", "STRUCT", "-C", "0.05", "-m", "-22", "-u"],
         "both_sum": ["-p", "SEQ", "-q", "STRUCT", "-C", "0.05", "-m", "-25", "--min-seqstruct", "-18", "--flank", "3"],
         "both_sum_alone": ["-p", "SEQ", "-q", "STRUCT", "-C", "0.05", "-m", " -inf", "--min-seqstruct", "-16", "-B", "BG"]}


@pytest.mark.parametrize("form", ["directory", "store"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_command_files_equal_those_of_the_restated_rules_byte_for_byte(engine, inputs, tmp_path, case, form, monkeypatch):
    from conftest import DATA_DIR
    from sites_helpers import RulesEngine
    fa, d, sdir = inputs
    bg = tmp_path / "bg.txt"
    bg.write_text(repr({c: 1.0 / 7 for c in "EHTBLRM"}))
    names = {"SEQ": os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt"),
             "STRUCT": os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_struct.txt"), "BG": str(bg)}
    argv = [names.get(a, a) for a in CASES[case]] + ([fa] if "-p" in CASES[case] else []) + [d if form == "directory" else sdir]
    monkeypatch.setenv("RNASCAN_BATCH_POSITIONS", "3000")              # several batches
    rc, want = _command(argv, RulesEngine(), str(tmp_path / "want"))
    assert rc == 0 and len(want) == (3 if "-p" in argv else 2) and want["counts"].count(b"\n") > 5
    rc, got = _command(argv, engine, str(tmp_path / "got"))
    assert rc == 0 and got == want
    monkeypatch.delenv("RNASCAN_BATCH_POSITIONS")
    rc, got = _command(argv, engine, str(tmp_path / "got1"))           # one batch
    assert rc == 0 and got == want


def test_command_names_the_bad_cell_under_a_site(engine, inputs, tmp_path, capfd):
    from conftest import DATA_DIR
    from rnascan_amd import store
    fa, d, sdir = inputs
    bad = str(tmp_path / "store")
    import shutil
    shutil.copytree(sdir, bad)
    ps = store.ProfileStore(bad)
    rows = np.array(ps.profile)
    rows[int(ps.offsets[7]) + 11, list(ps.letters).index("R")] = np.nan
    rows[int(ps.offsets[40]) + 2, 0] = -1.0
    del ps
    rows.tofile(os.path.join(bad, "profile.f64"))
    rc, files = _command(["-q", os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_struct.txt"), "-C", "0.05", "-m", "-18", "-u",
                          "--flank", "8", bad], engine, str(tmp_path / "x"))
    err = capfd.readouterr().err
    assert rc == 1 and files == {}
    assert "k07" in err and "position 12" in err and "column R" in err and "k40" not in err


@pytest.mark.timeout(600)
def test_command_on_two_ranks_of_the_one_gpu_writes_the_same_files(inputs, tmp_path):
    """`--gpus 2` as tests/test_gpu_launch.py rehearses it: two ranks share device 0"""
    import subprocess
    import sys
    from conftest import DATA_DIR, REPO
    fa, d, sdir = inputs
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["PYTHONPATH"] = os.pathsep.join([REPO] + [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    tail = ["-p", os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt"), "-q",
            os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_struct.txt"), "-C", "0.05", "-m", "-25", "--min-seqstruct", "-18",
            "--flank", "3", fa, sdir]
    cmd = [sys.executable, "-m", "rnascan_amd.sites"]
    one = subprocess.run(cmd + ["-o", str(tmp_path / "one")] + tail, env=env, capture_output=True, text=True, timeout=280)
    assert one.returncode == 0, one.stderr[-3000:]
    two = subprocess.run(cmd + ["-o", str(tmp_path / "two"), "--gpus", "2"] + tail, env=dict(env, RNASCAN_ONE_DEVICE="1"),
                         capture_output=True, text=True, timeout=280)
    assert two.returncode == 0, two.stderr[-3000:]
    for suffix in ("struct", "seq", "counts"):
        a = open("%s.%s.txt" % (tmp_path / "one", suffix), "rb").read()
        assert a.count(b"\n") == 1 + 18 + 6 and a == open("%s.%s.txt" % (tmp_path / "two", suffix), "rb").read()


def test_element_indices_beyond_2_31(engine):
    """float32 rows made on the device, 7 x rows > 2^31: the hits lie in the last record, whose cells have flat element
    indices that no 32-bit integer holds; the expected sums come from the rules on that record's rows alone"""
    import torch
    from rnascan_amd import pack
    if torch.cuda.mem_get_info()[0] < 12e9:
        pytest.skip("needs 12 GB of free HBM")
    ctx = engine.ctx
    dev = torch.device("cuda", 0)
    m, flank, tail = 12, 5, 700
    W = m + 2 * flank
    n_pos = (1 << 31) // 7 + 5000
    g = torch.Generator(device=dev)
    g.manual_seed(6)
    prof = torch.randint(0, 1024, (n_pos, 7), device=dev, generator=g, dtype=torch.int32).to(torch.float32) / 1024.0
    first = n_pos - tail - 1                                           # the last record: rows [first, first + tail)
    assert first * 7 > (1 << 31)
    offsets = np.asarray([0, first], dtype=np.int64)
    lengths = np.asarray([first - 1, tail], dtype=np.int64)
    local = pack.Stream(None, prof[first:first + tail + 1].cpu().numpy(), np.asarray([0]), np.asarray([tail]))
    start = np.asarray([0, 1, 2, 3, 4, 9, 300, 301, tail - m - 1, tail - m], dtype=np.int64)
    _, want, _ = rules.site_sums(local.profile, None, start, local.offsets, local.lengths, m, flank)
    pos = start + first
    grp_first, grp_rec = np.asarray([0, pos.size], dtype=np.int64), np.asarray([1], dtype=np.int64)
    up = lambda a: torch.from_numpy(a).to(dev)                         # noqa: E731
    d_pos, gf, gr, off, ln = up(pos), up(grp_first), up(grp_rec), up(offsets), up(lengths)
    sums = torch.full((1, W, 7), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.site_sums_dev(None, prof.data_ptr(), np.float32, n_pos, d_pos.data_ptr(), pos.size, gf.data_ptr(), gr.data_ptr(), 1,
                      off.data_ptr(), ln.data_ptr(), 2, m, flank, sums.data_ptr(), None)
    ctx.synchronize()
    assert np.array_equal(bits(sums.cpu().numpy()), bits(want))
    # a bad cell there is named by its 64-bit element index
    prof[first + 302, 3] = float("nan")
    torch.cuda.synchronize()
    with pytest.raises(ValueError) as e:
        ctx.site_sums_dev(None, prof.data_ptr(), np.float32, n_pos, d_pos.data_ptr(), pos.size, gf.data_ptr(), gr.data_ptr(), 1,
                          off.data_ptr(), ln.data_ptr(), 2, m, flank, sums.data_ptr(), None)
    assert e.value.element == (first + 302) * 7 + 3 and e.value.element > (1 << 31)
    del prof
    torch.cuda.empty_cache()
