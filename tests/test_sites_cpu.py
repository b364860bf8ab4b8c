"""Site profiles without a GPU: pfmscan_site_groups against the restated rules (tests/sites_rules.py), known answers, the
reference's struct_pfm_from_aligned + norm_pfm on one-hot inputs (tests/golden/sites/), the invariance of the result under
batches, record order and ranks, the command's files, and the host-only native code under the sanitizers."""
import ctypes
import gzip
import io
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sites_rules as rules
from background_helpers import COLUMNS, as_ranks, one_hot, random_rows, write_fasta, write_profile
from conftest import DATA_DIR, GOLDEN_DIR, REPO
from sites_helpers import RulesEngine, site_windows, write_inputs as _inputs
from rnascan_amd import _lib, cli, fasta, pack, pssm, sites, store

SEQ_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt")
STRUCT_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_struct.txt")
C1_FASTA = os.path.join(DATA_DIR, "HIST2H3C_3p_end.fa")
C1_PROFILE = os.path.join(DATA_DIR, "HIST2H3C_3p_end_structure.txt")
from sites_helpers import SITE  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def read_pfm(path):
    """(letters, float64 [rows][letters]) of a PFM file, every number through float() as -p / -q read it"""
    cols = pssm.read_pfm(path)
    return list(cols), np.stack(list(cols.values()), axis=1)


# ---- 1. the groups -----------------------------------------------------------------------------------------------------
def _table(rng, lengths):
    lengths = np.asarray(lengths, dtype=np.int64)
    offsets = np.zeros(lengths.size, dtype=np.int64)
    if lengths.size > 1:
        offsets[1:] = np.cumsum(lengths[:-1] + 1)
    return offsets, lengths


def _windows(offsets, lengths, m):
    return np.concatenate([np.arange(o, o + max(L - m + 1, 0)) for o, L in zip(offsets, lengths)] + [np.zeros(0, np.int64)]).astype(np.int64)


def test_groups_equal_the_rules_on_random_hit_lists():
    rng = np.random.default_rng(1)
    for it in range(60):
        m = int(rng.integers(1, 20))
        offsets, lengths = _table(rng, rng.integers(0, 120, size=int(rng.integers(1, 30))))
        win = _windows(offsets, lengths, m)
        pos = win[rng.random(win.size) < rng.choice([0.02, 0.3, 1.0])]
        got = _lib.site_groups(pos, offsets, lengths, m)
        want = rules.groups(pos, offsets, lengths, m)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_groups_of_exactly_4096_4097_and_two_full_groups_and_three():
    m = 5
    sizes = [3, 4096, 4097, 2 * 4096 + 3, 0, 1]
    offsets, lengths = _table(None, [n + m - 1 if n else 2 for n in sizes])
    pos = _windows(offsets, lengths, m)
    first, rec = _lib.site_groups(pos, offsets, lengths, m)
    assert np.diff(first).tolist() == [3, 4096, 4096, 1, 4096, 4096, 3, 1]
    assert rec.tolist() == [0, 1, 2, 2, 3, 3, 3, 5]
    want = rules.groups(pos, offsets, lengths, m)
    assert np.array_equal(first, want[0]) and np.array_equal(rec, want[1])
    # hits of the first and of the last record only; an empty list
    for keep in (pos[:3], pos[-1:], pos[:0]):
        got, want = _lib.site_groups(keep, offsets, lengths, m), rules.groups(keep, offsets, lengths, m)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert _lib.site_groups(pos[:0], offsets, lengths, m)[0].tolist() == [0]
    # groups are anchored at the RECORD's first hit: dropping hits of other records moves no cut of record 3
    only = pos[pos >= offsets[3]]
    assert np.diff(_lib.site_groups(only, offsets, lengths, m)[0]).tolist() == [4096, 4096, 3, 1]


def test_groups_reject_what_the_definition_excludes():
    offsets, lengths = np.asarray([0, 11, 30]), np.asarray([10, 18, 5])
    ok = np.asarray([0, 7, 11, 26, 30, 32])
    _lib.site_groups(ok, offsets, lengths, 3)
    for pos, off, ln in [([7, 0], offsets, lengths),                       # descending
                         ([0, 7, 7], offsets, lengths),                    # equal
                         ([0, 8], offsets, lengths),                       # a window across the separator
                         ([10], offsets, lengths),                         # a window that starts on the separator
                         ([0, 33], offsets, lengths),                      # a window past the stream
                         ([0, 40], offsets, lengths),
                         ([-1], offsets, lengths),
                         ([0], [0, 10, 30], lengths),                      # a record on the separator of the one before
                         ([0], [0, 30, 11], lengths),
                         ([0], [-1, 11, 30], lengths),
                         ([0], offsets, [10, -1, 5]),
                         ([0], offsets, [10, 19, 5])]:
        with pytest.raises(ValueError):
            _lib.site_groups(pos, off, ln, 3)
        with pytest.raises(ValueError):
            rules.groups(np.asarray(pos), np.asarray(off), np.asarray(ln), 3)
    with pytest.raises(ValueError):
        _lib.site_groups(ok, offsets, lengths, 0)


def test_groups_capacity_protocol():
    L = _lib.load()
    offsets, lengths = _table(None, [20, 9000, 7])
    pos = _windows(offsets, lengths, 4)
    want = rules.groups(pos, offsets, lengths, 4)
    n = ctypes.c_int64(-1)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                        # noqa: E731
    for cap in (0, 1, want[1].size - 1):
        first = np.full(cap + 1, -5, dtype=np.int64)
        rec = np.full(max(cap, 1), -5, dtype=np.int64)
        rc = L.pfmscan_site_groups(p(pos), pos.size, p(offsets), p(lengths), 3, 4, cap, p(first), p(rec), ctypes.byref(n))
        assert rc == _lib.E_CAPACITY and n.value == want[1].size
        assert (first == -5).all() and (rec == -5).all()                   # nothing was written
    first = np.full(want[1].size + 3, -5, dtype=np.int64)
    rec = np.full(want[1].size + 2, -5, dtype=np.int64)
    rc = L.pfmscan_site_groups(p(pos), pos.size, p(offsets), p(lengths), 3, 4, want[1].size + 2, p(first), p(rec), ctypes.byref(n))
    assert rc == 0 and n.value == want[1].size
    assert np.array_equal(first[:n.value + 1], want[0]) and np.array_equal(rec[:n.value], want[1])


def test_the_library_exports_the_site_entry_points():
    L = _lib.load()
    assert _lib.ABI_VERSION >= 15 and L.pfmscan_abi_version() == _lib.ABI_VERSION
    for name in ("pfmscan_site_groups", "pfmscan_site_sums_dev", "pfmscan_site_sums_staged", "pfmscan_site_sums_host"):
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    header = open(os.path.join(REPO, "include", "pfmscan.h")).read()
    assert "((w0 + w1) + w2) + w3" in header and "PFMSCAN_SITE_GROUP 4096" in header and rules.GROUP == _lib.SITE_GROUP == 4096


# ---- 2. known answers --------------------------------------------------------------------------------------------------
def _sum_up(engine, stream, pos, m, flank=0, cols=COLUMNS, letters=True):
    rows = sites.Rows(m + 2 * flank, profile=True, letters=letters and stream.codes is not None)
    sites.accumulate(engine, rows, stream, ["r%d" % i for i in range(len(stream.offsets))], lambda r: list(cols), pos, m, flank)
    return sites.combine(rows)


def test_one_hit_gives_the_profile_rows_under_it_bit_for_bit():
    _, prof = fasta.read_profile(C1_PROFILE)
    st = pack.pack(profiles=[prof], profile_dtype=np.float64)
    for start, m, flank in ((17, 18, 0), (0, 9, 0), (prof.shape[0] - 9, 9, 0), (3, 5, 3)):
        S, counts, cov, hits = _sum_up(RulesEngine(), st, np.asarray([start]), m, flank)
        assert hits == 1 and counts is None and (cov == 1).all()
        assert np.array_equal(bits(S), bits(prof[start - flank:start + m + flank]))


def _c1_dir(tmp_path):
    d = tmp_path / "avg"
    d.mkdir()
    shutil.copy(C1_PROFILE, str(d / "structure.hg19_dna.txt"))
    return str(d)


def _run(argv, engine=None):
    """the command in this process on the restated rules -> (exit code, {suffix: file bytes})"""
    prefix = argv[argv.index("-o") + 1]
    rc = sites.main(list(argv), engine=engine or RulesEngine())
    out = {}
    for suffix in ("struct", "seq", "counts"):
        path = "%s.%s.txt" % (prefix, suffix)
        if os.path.exists(path):
            out[suffix] = open(path, "rb").read()
    return rc, out


def test_the_command_on_the_c1_inputs_one_site_is_its_rows_normalised(tmp_path, capfd):
    d = _c1_dir(tmp_path)
    prefix = str(tmp_path / "out")
    rc, files = _run(["-p", SEQ_PFM, "-u", "-o", prefix, C1_FASTA, d])
    assert rc == 0 and sorted(files) == ["counts", "seq", "struct"]
    assert "Found 1 sites" in capfd.readouterr().err
    # where rnascan itself finds the site
    table = io.StringIO()
    cli.main(["-p", SEQ_PFM, "-u", C1_FASTA], engine=RulesEngine(), out=table)
    row = table.getvalue().splitlines()[1].split("\t")
    start, end, site = int(row[3]), int(row[4]), row[5]
    _, prof = fasta.read_profile(C1_PROFILE)
    rows = prof[start - 1:end]
    total = np.zeros(rows.shape[0])
    for c in range(7):
        total = total + rows[:, c]
    letters, got = read_pfm(prefix + ".struct.txt")
    assert "".join(letters) == "BEHLMRT"
    assert np.array_equal(bits(got), bits(rows / total[:, None]))
    letters, seq = read_pfm(prefix + ".seq.txt")
    assert "".join(letters) == "ACGU"
    assert "".join("ACGU"[k] for k in np.argmax(seq, axis=1)) == site and set(np.unique(seq)) == {0.0, 1.0}
    # --flank 0 output loads as a motif, and rnascan scans with it
    pm = cli.load_motif(prefix + ".struct.txt", 0, fasta.STRUCT, None)
    assert list(pm.values())[0].length == end - start + 1
    again = io.StringIO()
    cli.main(["-q", prefix + ".struct.txt", "-u", "-C", "0.01", "-m", "1", d], engine=RulesEngine(), out=again)
    assert any(ln.split("\t")[3] == str(start) for ln in again.getvalue().splitlines()[1:])
    assert len(cli.load_motif(prefix + ".seq.txt", 0, fasta.RNA, None)) == 1


# ---- 3. one-hot rows: integer counts, and the reference's PFM ------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_sites():
    with gzip.open(os.path.join(GOLDEN_DIR, "sites", "sites.json.gz")) as f:
        g = json.load(f)
    recs = g["records"]
    st = pack.pack(code_arrays=[pack.encode_rna(s) for _, s, _ in recs], profiles=[one_hot(t) for _, _, t in recs],
                   profile_dtype=np.float64)
    pos = np.sort(np.asarray([st.offsets[r] + s for r, s in g["sites"]], dtype=np.int64))
    return g, st, pos


@pytest.mark.parametrize("flank", [0, 3])
def test_one_hot_rows_give_the_reference_pfm_number_for_number(golden_sites, flank):
    g, st, pos = golden_sites
    m = g["m"]
    assert max(np.diff(rules.groups(pos, st.offsets, st.lengths, m)[0])) == 4096        # a record with more than one group
    S, counts, cov, hits = _sum_up(RulesEngine(), st, pos, m, flank)
    assert hits == len(g["sites"])
    want_counts = np.asarray([g["counts"][str(flank)][c] for c in COLUMNS], dtype=np.float64).T
    assert np.array_equal(S, want_counts)                                                # sums of one-hot rows are integer counts
    struct, seq, foreign = sites.site_pfms(S, counts)
    want = np.asarray([[float.fromhex(x) for x in g["pfm"][str(flank)][c]] for c in COLUMNS]).T
    assert np.array_equal(bits(struct), bits(want))
    assert np.array_equal(S.sum(axis=1), cov) and np.array_equal(counts.sum(axis=1), cov) and not foreign.any()
    # the letters: counted straight from the strings
    x, counted = site_windows(st, pos, m, flank)
    for k in range(4):
        assert np.array_equal(counts[:, k], ((st.codes[np.where(counted, x, 0)] == k) & counted).sum(axis=0))


# ---- 4. invariance -------------------------------------------------------------------------------------------------------
def _args(argv):
    return sites.getoptions(argv)


def _gather(argv, rank=0, world=1, dist=None, engine=None):
    args = _args(argv)
    engine = engine or RulesEngine()
    seq = cli.load_motif(args.pfm_seq, args.pseudocount, fasta.RNA, None) if args.pfm_seq else None
    st = cli.load_motif(args.pfm_struct, args.pseudocount, fasta.STRUCT, None) if args.pfm_struct else None
    return sites.gather(engine, args, seq, st, rank, world, dist)


def _same(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and (a[1] is None) == (b[1] is None) and \
        (a[1] is None or np.array_equal(a[1], b[1])) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_result_does_not_depend_on_batches_input_form_or_ranks(tmp_path, monkeypatch):
    fa, d, sdir = _inputs(tmp_path)
    base = ["-p", SEQ_PFM, "-m", "4", "--flank", "5", "-o", str(tmp_path / "x"), fa]
    one = _gather(base + [d])
    assert one[3] > 25 and one[2].min() < one[3] and one[2].max() == one[3]      # some flank columns were skipped
    for batch in ("1", "300", "2000"):
        monkeypatch.setenv("RNASCAN_BATCH_POSITIONS", batch)
        assert _same(_gather(base + [d]), one) and _same(_gather(base + [sdir]), one)
    monkeypatch.delenv("RNASCAN_BATCH_POSITIONS")
    for src in (d, sdir):
        for world in (2, 3):
            got = as_ranks(world, lambda r, w, dist: _gather(base + [src], r, w, dist))
            assert all(isinstance(g, tuple) and _same(g, one) for g in got), got
    # -q only and both PFMs, directory against store
    for extra in (["-q", STRUCT_PFM, "-C", "0.05", "-m", "-14"],
                  ["-p", SEQ_PFM, "-q", STRUCT_PFM, "-C", "0.05", "-m", "-25", "--min-seqstruct", "-18"]):
        argv = extra + ["-o", str(tmp_path / "y")] + ([fa] if "-p" in extra else [])
        a, b = _gather(argv + [d]), _gather(argv + [sdir])
        assert a[3] > 5 and _same(a, b)
        got = as_ranks(3, lambda r, w, dist: _gather(argv + [sdir], r, w, dist))
        assert all(isinstance(g, tuple) and _same(g, a) for g in got), got


def test_record_order_does_not_change_the_bits(tmp_path):
    """the same records in another order: other streams, other groups order -- math.fsum sees the same multiset of rows"""
    fa, d, sdir = _inputs(tmp_path)
    recs = list(fasta.open_lazy(fa))
    other = str(tmp_path / "reversed.fa")
    write_fasta(other, [(r.id, r.seq) for r in reversed(recs)])
    base = ["-p", SEQ_PFM, "-m", "4", "--flank", "2", "-o", str(tmp_path / "x")]
    one = _gather(base + [fa, d])
    assert _same(_gather(base + [other, d]), one) and _same(_gather(base + [other, sdir]), one)


def _bad_store(tmp_path, cells):
    """the store of _inputs with cells overwritten: (record index, 0-based row, letter, value)"""
    fa, d, sdir = _inputs(tmp_path)
    ps = store.ProfileStore(sdir)
    rows = np.array(ps.profile)
    for rec, row, letter, value in cells:
        rows[int(ps.offsets[rec]) + row, COLUMNS.index(letter)] = value
    del ps
    rows.tofile(os.path.join(sdir, "profile.f64"))
    return fa, sdir


def test_a_bad_cell_under_a_site_names_record_position_and_letter(tmp_path):
    # -q hits at a low -m lie nearly everywhere, and their flanks cover the rest
    fa, sdir = _bad_store(tmp_path, [(20, 6, "M", np.nan), (3, 4, "H", -0.5), (3, 9, "B", np.inf)])
    argv = ["-q", STRUCT_PFM, "-C", "0.05", "-m", "-18", "--flank", "8", "-u", "-o", str(tmp_path / "x"), sdir]
    with pytest.raises(sites.SitesError) as e:
        _gather(argv)
    assert (e.value.record, e.value.position, e.value.letter, e.value.value) == ("k03", 5, "H", -0.5)
    assert "k03" in str(e.value) and "position 5" in str(e.value) and "column H" in str(e.value)
    import pickle
    again = pickle.loads(pickle.dumps(e.value))
    assert isinstance(again, sites.SitesError) and str(again) == str(e.value) and again.position == 5
    # every rank raises the earliest one, also the ranks whose own share is clean or fails later
    for world in (2, 3):
        got = as_ranks(world, lambda r, w, dist: _gather(argv, r, w, dist))
        for g in got:
            assert isinstance(g, sites.SitesError) and (g.record, g.position, g.letter) == ("k03", 5, "H"), g
    # the command: exit code 1, the message on stderr, no files
    rc, files = _run(argv)
    assert rc == 1 and files == {}


def test_a_bad_cell_under_no_site_is_no_error(tmp_path):
    fa, sdir = _bad_store(tmp_path, [(1, 0, "M", np.nan)])                   # k01 holds no site of the sequence motif
    base = ["-p", SEQ_PFM, "-m", "6", "-o", str(tmp_path / "x"), fa]
    got = _gather(base + [sdir])
    assert got[3] > 10 and np.isfinite(got[0]).all()


def _gloo_worker(rank, world, port, outdir, argv):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1",
                       "MASTER_PORT": str(port), "RNASCAN_DIST_BACKEND": "gloo", "RNASCAN_ONE_DEVICE": "1"})
    from sites_helpers import RulesEngine
    from rnascan_amd import sites
    rc = sites.main(argv, engine=RulesEngine())
    with open(os.path.join(outdir, "rc.%d" % rank), "w") as f:
        f.write(str(rc))
    import torch.distributed as dist
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_the_command_under_two_gloo_ranks_writes_the_same_files(tmp_path):
    import socket
    import torch.multiprocessing as mp
    fa, d, sdir = _inputs(tmp_path)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    tail = ["-p", SEQ_PFM, "-q", STRUCT_PFM, "-C", "0.05", "-m", "-25", "--min-seqstruct", "-18", "--flank", "3", fa, sdir]
    rc, one = _run(["-o", str(tmp_path / "one")] + tail)
    assert rc == 0 and len(one) == 3
    mp.spawn(_gloo_worker, args=(2, port, str(tmp_path), ["-o", str(tmp_path / "two")] + tail), nprocs=2, join=True)
    assert open(tmp_path / "rc.0").read() == "0" and open(tmp_path / "rc.1").read() == "0"
    for suffix, want in one.items():
        assert open("%s.%s.txt" % (tmp_path / "two", suffix), "rb").read() == want


# ---- 5. coverage ---------------------------------------------------------------------------------------------------------
def test_coverage_from_positions_equals_the_sum_of_counts():
    rng = np.random.default_rng(9)
    m, flank = 4, 6                                                        # W = 16: the records of 4, 5 and 9 are shorter
    lengths = [4, 5, 9, 16, 40, 17, 4]
    st = pack.pack(code_arrays=[rng.integers(0, 6, size=L).astype(np.uint8) for L in lengths],
                   profiles=[random_rows(rng, L) for L in lengths], profile_dtype=np.float64)
    pos = np.flatnonzero(st.window_mask(m))
    cov = sites.coverage(st, pos, m, flank)
    assert np.array_equal(cov, rules.coverage(pos, st.offsets, st.lengths, m, flank))
    _, sums, counts = RulesEngine().site_sums(st, pos, m, flank)
    assert np.array_equal(counts.astype(np.int64).sum(axis=(0, 2)), cov)
    assert cov[flank:flank + m].tolist() == [pos.size] * m and cov[0] < pos.size and cov[-1] < pos.size
    x, counted = site_windows(st, pos, m, flank)
    assert np.array_equal(counted.sum(axis=0), cov)
    # rows sum to 1 here, so the structure mass of a column is its coverage too
    S = rules.total(sums)
    assert np.allclose(S.sum(axis=1), cov, rtol=1e-12)
    # foreign letters (codes 4 .. 7 inside a record) are reported, not counted into the PFM
    total = counts.astype(np.int64).sum(axis=0)
    _, seq, foreign = sites.site_pfms(None, total)
    assert foreign.sum() > 0 and np.array_equal(foreign, total[:, 4:].sum(axis=1)) and np.allclose(seq.sum(axis=1), 1.0)


def test_a_column_without_mass_is_an_error_that_names_it():
    S = np.ones((5, 7))
    S[3] = 0.0
    with pytest.raises(sites.InputError) as e:
        sites.site_pfms(S, None)
    assert "column 3" in str(e.value)


# ---- 6. column orders of a directory ---------------------------------------------------------------------------------------
def test_files_with_their_own_column_orders_are_matched_by_name(tmp_path):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    fa, d1, _ = _inputs(tmp_path / "a")
    fa2, d2, _ = _inputs(tmp_path / "b", orders=["BEHLMRT", "TRMLHEB", "EHTBLRM", "BEHLMRT", "MBTEHLR"])
    assert open(fa).read() == open(fa2).read()
    for extra in (["-p", SEQ_PFM, "-m", "4"], ["-p", SEQ_PFM, "-q", STRUCT_PFM, "-C", "0.05", "-m", "-22", "-u"]):
        base = extra + ["--flank", "2", "-o", str(tmp_path / "x"), fa]
        want = _gather(base + [d1])
        assert want[3] > 5 and _same(_gather(base + [d2]), want)
        got = as_ranks(2, lambda r, w, dist: _gather(base + [d2], r, w, dist))
        assert all(isinstance(g, tuple) and _same(g, want) for g in got), got


# ---- 7. the command's edges ------------------------------------------------------------------------------------------------
def test_zero_hits_exit_1_and_write_nothing(tmp_path, capfd):
    d = _c1_dir(tmp_path)
    rc, files = _run(["-p", SEQ_PFM, "-u", "-m", "50", "-o", str(tmp_path / "none"), C1_FASTA, d])
    assert rc == 1 and files == {}
    assert "Found 0 sites" in capfd.readouterr().err


def test_fasta_and_profiles_must_pair_one_to_one(tmp_path, capfd):
    fa, d, _ = _inputs(tmp_path, n=6)
    prefix = ["-p", SEQ_PFM, "-u", "-m", "4", "-o", str(tmp_path / "x")]
    os.rename(os.path.join(d, "structure.k02.txt"), os.path.join(d, "structure.other.txt"))
    rc, files = _run(prefix + [fa, d])
    assert rc == 1 and files == {} and "k02" in capfd.readouterr().err
    os.rename(os.path.join(d, "structure.other.txt"), os.path.join(d, "structure.k02.txt"))
    _, prof = fasta.read_profile(os.path.join(d, "structure.k04.txt"))
    write_profile(os.path.join(d, "structure.k04.txt"), prof[:-1])
    rc, files = _run(prefix + [fa, d])
    err = capfd.readouterr().err
    assert rc == 1 and files == {} and "k04" in err and "rows" in err


def test_flank_output_is_w_columns_wide_and_help_says_it_is_no_pfm_for_q(tmp_path):
    fa, d, _ = _inputs(tmp_path)
    rc, files = _run(["-p", SEQ_PFM, "-m", "4", "--flank", "7", "-o", str(tmp_path / "f"), fa, d])
    assert rc == 0
    assert files["struct"].count(b"\n") == 1 + len(SITE) + 14 and files["struct"].startswith(b"PO\tB\tE\tH\tL\tM\tR\tT\n")
    assert files["seq"].startswith(b"PO\tA\tC\tG\tU\n")
    assert files["counts"].splitlines()[0].split(b"\t")[:3] == [b"PO", b"Sites", b"Coverage"]
    # every number reads back to the float64 it was: the shortest round-tripping form
    _, got = read_pfm(str(tmp_path / "f") + ".struct.txt")
    S = _gather(["-p", SEQ_PFM, "-m", "4", "--flank", "7", "-o", "unused", fa, d])[0]
    assert np.array_equal(bits(got), bits(sites.site_pfms(S, None)[0]))
    for line in files["struct"].splitlines()[1:]:
        for tok in line.split(b"\t")[1:]:
            assert tok.decode() == repr(float(tok))
    with pytest.raises(SystemExit):
        sites.getoptions(["--help"])


def test_help_text(capsys):
    with pytest.raises(SystemExit):
        sites.getoptions(["--help"])
    assert "not a PFM for -q" in " ".join(capsys.readouterr().out.split())


# ---- 8. the host-only native code under the sanitizers -------------------------------------------------------------------
def test_site_groups_under_sanitizers(tmp_path):
    """pfmscan_sites_host.hip has no device code: compiled with g++ -fsanitize=address,undefined beside a stand-alone driver
    (tests/c/fuzz_sites.cpp, its own main) that feeds it random and adversarial tables in exact-size heap buffers and checks
    every answer against the definition: no overread, no overflow, no UB"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "fuzz_sites")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tests", "c", "fuzz_sites.cpp"),
           "-x", "c++", os.path.join(REPO, "rnascan_amd", "csrc", "pfmscan_sites_host.hip"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().startswith("ok"), (run.stdout + run.stderr)[-3000:]
