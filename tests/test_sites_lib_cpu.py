"""Site profiles of a motif library without a GPU: the long accumulator's host half (decomposition, add, round) against
math.fsum and the Python-int restatement (tests/sites_lib_rules.py), the motif-major groups and order against the rules,
``sites --all-motifs`` on the rules engine against one single-motif run per pair, byte for byte, its invariance under
batches, input form, record order and ranks, and the host-only native code under the sanitizers."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import sites_lib_helpers as helpers
import sites_lib_rules as lrules
import sites_rules as rules
from background_helpers import as_ranks, write_fasta
from conftest import REPO
from sites_lib_helpers import RulesEngine
from rnascan_amd import _lib, cli, fasta, sites

DBL_MAX = 1.7976931348623157e308
MIN_NORMAL = 2.0 ** -1022
MAX_SUBNORMAL = MIN_NORMAL - 5e-324


def fsum(values):
    try:
        return math.fsum(values)
    except OverflowError:
        return math.inf


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def check_list(values):
    """limbs == the Python-int restatement, bit for bit; rounded == math.fsum, raw and normalised"""
    acc = _lib.site_acc_from_doubles(values)
    assert [int(x) for x in acc] == lrules.raw_limbs(values)
    assert lrules.limbs_int(acc) == sum(lrules.as_int(v) for v in values)
    want = fsum(values)
    got = _lib.site_acc_round(acc.reshape(lrules.LIMBS, 1))[0]
    assert bits(got) == bits(want), (values[:8], got, want)
    assert bits(lrules.round_int(lrules.limbs_int(acc))) == bits(want)
    norm = _lib.site_acc_add(np.zeros((lrules.LIMBS, 1), dtype=np.uint64), acc.reshape(lrules.LIMBS, 1))
    assert lrules.normalised(norm) and lrules.limbs_int(norm[:, 0]) == lrules.limbs_int(acc)
    assert bits(_lib.site_acc_round(norm)[0]) == bits(want)


# ---- 1. the decomposition and the rounding -------------------------------------------------------------------------------
def test_named_values_and_ties_to_even():
    ulp = 2.0 ** -52
    for values in ([5e-324], [MAX_SUBNORMAL], [MIN_NORMAL], [1.0], [1.0 + ulp], [DBL_MAX], [0.0], [], [0.0, 5e-324, 0.0],
                   [MAX_SUBNORMAL, 5e-324], [5e-324] * 7, [DBL_MAX, 5e-324], [1.0, DBL_MAX, MIN_NORMAL, 5e-324, 1e-300, 1e300]):
        check_list(values)
    # half-way cases: 1 + half an ulp is a tie (to even: down), 1 + ulp + half an ulp a tie (up), a crumb more breaks it
    for e in (-1000, -52, 0, 1, 52, 53, 500, 1000):
        s = 2.0 ** e
        half = s * ulp / 2
        assert fsum([s, half]) == s and fsum([s * (1 + ulp), half]) == s * (1 + 2 * ulp)
        for values in ([s, half], [s * (1 + ulp), half], [s, half, s * 2.0 ** -1000 if e > -50 else 5e-324],
                       [s * (1 + ulp), half / 2, half / 2], [s, half / 2, half / 4], [s] * 3 + [half] * 3):
            check_list(values)
    # a tie at the edge of the subnormals, and one that rounds up into the next binade
    check_list([MAX_SUBNORMAL, MIN_NORMAL, 5e-324])
    check_list([2.0 - ulp, ulp / 2])
    assert _lib.site_acc_from_doubles([5e-324])[0] == 1 and not _lib.site_acc_from_doubles([5e-324])[1:].any()
    assert _lib.site_acc_from_doubles([DBL_MAX])[lrules.LIMBS - 1] != 0


def test_ten_thousand_random_values_of_mixed_exponents():
    rng = np.random.default_rng(1)
    raw = (rng.integers(0, 2047, size=10000).astype(np.uint64) << np.uint64(52)) | rng.integers(0, 1 << 52, size=10000).astype(np.uint64)
    values = raw.view(np.float64)
    assert np.isfinite(values).all() and (values == 0).sum() < 3 and (values < MIN_NORMAL).any() and (values > 1e300).any()
    # the whole range at once would overflow: lists of mixed exponents below 2^1000, and short ones over the whole range
    small = values[values < 2.0 ** 1000]
    check_list(small.tolist())
    for a in range(0, 10000, 25):
        check_list(values[a:a + int(rng.integers(1, 25))].tolist())
    # neighbouring exponents: cancellation-free sums with long carry chains
    for e in (1, 31, 32, 33, 64, 1023, 2014, 2045):
        near = ((np.uint64(e) + rng.integers(0, 2, size=300).astype(np.uint64)) << np.uint64(52)) | rng.integers(0, 1 << 52, size=300).astype(np.uint64)
        check_list(near.view(np.float64).tolist())
        check_list([float(np.uint64(e << 52).view(np.float64))] * 1000 + [float(np.nextafter(np.uint64(e << 52).view(np.float64), np.inf))] * 999)


def test_overflow_rounds_to_infinity_and_bad_values_are_refused():
    for values in ([DBL_MAX, DBL_MAX], [DBL_MAX, 2.0 ** 970], [DBL_MAX] * 1000, [1.5e308, 1.5e308]):
        assert fsum(values) == math.inf
        check_list(values)
    check_list([DBL_MAX, 2.0 ** 969])                                    # a tie below the edge: stays DBL_MAX
    assert fsum([DBL_MAX, 2.0 ** 969]) == DBL_MAX
    for bad in (-1.0, -5e-324, math.inf, -math.inf, math.nan):
        with pytest.raises(ValueError):
            _lib.site_acc_from_doubles([1.0, bad])
    check_list([-0.0, 1.0])


# ---- 2. site_acc_add -----------------------------------------------------------------------------------------------------
def test_a_split_list_merged_is_the_whole_list_and_stays_normalised():
    rng = np.random.default_rng(2)
    n_acc, n_cells, per = 3, 5, 40
    raw = (rng.integers(0, 2040, size=(n_acc, n_cells, per)).astype(np.uint64) << np.uint64(52)) | \
        rng.integers(0, 1 << 52, size=(n_acc, n_cells, per)).astype(np.uint64)
    values = raw.view(np.float64)

    def acc_of(a, b):
        out = np.zeros((n_acc, lrules.LIMBS, n_cells), dtype=np.uint64)
        for k in range(n_acc):
            for e in range(n_cells):
                out[k, :, e] = _lib.site_acc_from_doubles(values[k, e, a:b])
        return out

    whole = _lib.site_acc_add(np.zeros((n_acc, lrules.LIMBS, n_cells), dtype=np.uint64), acc_of(0, per))
    assert lrules.normalised(whole)
    for cuts in ([0, 13, per], [0, 1, 2, 39, per], [0, 0, 20, 20, per]):
        total = np.zeros_like(whole)
        for a, b in zip(cuts[:-1], cuts[1:]):
            part = acc_of(a, b)
            if a % 2:                                  # raw and normalised sources alike
                part = _lib.site_acc_add(np.zeros_like(part), part)
            assert _lib.site_acc_add(total, part) is total and lrules.normalised(total)
        assert np.array_equal(total, whole)
    S = _lib.site_acc_round(whole)
    for k in range(n_acc):
        for e in range(n_cells):
            assert bits(S[k, e]) == bits(fsum(values[k, e].tolist()))
    # many DBL_MAX: the top limb takes what no double holds, and still adds exactly
    top = _lib.site_acc_add(np.zeros((lrules.LIMBS, 1), dtype=np.uint64), _lib.site_acc_from_doubles([DBL_MAX] * 3).reshape(-1, 1))
    for _ in range(15):
        _lib.site_acc_add(top, top.copy())
    assert lrules.normalised(top) and lrules.limbs_int(top[:, 0]) == 3 * 2 ** 15 * lrules.as_int(DBL_MAX) and top[-1, 0] >= 1 << 32
    assert _lib.site_acc_round(top)[0] == math.inf
    with pytest.raises(ValueError):
        _lib.site_acc_add(np.zeros((3, 2), dtype=np.uint64), np.zeros((3, 2), dtype=np.uint64))


# ---- 3. groups and order of a library hit list ---------------------------------------------------------------------------
def _table(lengths):
    lengths = np.asarray(lengths, dtype=np.int64)
    offsets = np.zeros(lengths.size, dtype=np.int64)
    if lengths.size > 1:
        offsets[1:] = np.cumsum(lengths[:-1] + 1)
    return offsets, lengths


def _windows(offsets, lengths, m):
    return np.concatenate([np.arange(o, o + max(L - m + 1, 0)) for o, L in zip(offsets, lengths)] + [np.zeros(0, np.int64)]).astype(np.int64)


def _same_groups(pos, mot, n_motifs, off, ln, m):
    got = _lib.site_groups_lib(pos, mot, n_motifs, off, ln, m)
    want = lrules.groups(pos, mot, n_motifs, off, ln, m)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    return got


def test_groups_and_order_equal_the_rules_on_random_lists():
    rng = np.random.default_rng(3)
    for it in range(150):
        m, n_motifs = int(rng.integers(1, 9)), int(rng.integers(1, 7))
        off, ln = _table(rng.integers(0, 30, size=int(rng.integers(0, 7))))
        win = _windows(off, ln, m)
        empty = set(rng.choice(n_motifs, size=int(rng.integers(0, n_motifs)), replace=False).tolist())
        if it % 3 == 0:
            empty |= {0, n_motifs - 1, n_motifs // 2}                 # empty motifs first, middle and last
        parts = [win[rng.random(win.size) < rng.choice([0.2, 0.7, 1.0])] if k not in empty else win[:0] for k in range(n_motifs)]
        pos = np.concatenate(parts) if parts else win[:0]
        mot = np.concatenate([np.full(p.size, k, dtype=np.int32) for k, p in enumerate(parts)]) if parts else np.zeros(0, np.int32)
        gf, gr, gm = _same_groups(pos, mot, n_motifs, off, ln, m)
        assert gf[-1] == pos.size and not (set(gm.tolist()) & empty)
        # the (position, motif) order of the library scans -> motif-major, stably
        scan = np.lexsort((mot, pos))
        order = _lib.site_order_lib(pos[scan], mot[scan], n_motifs)
        assert np.array_equal(order, lrules.motif_major(pos[scan], mot[scan]))
        assert np.array_equal(pos[scan][order], pos) and np.array_equal(mot[scan][order], mot)


def test_motif_record_runs_of_4096_4097_and_two_full_groups_and_three():
    m = 3
    off, ln = _table([4096 + m - 1, 4097 + m - 1, 2 * 4096 + 3 + m - 1, 5])
    win = _windows(off, ln, m)
    pos = np.concatenate([win[:0], win, win[::2], win[:0]])
    mot = np.concatenate([np.full(win.size, 1, dtype=np.int32), np.full(win[::2].size, 2, dtype=np.int32)])
    gf, gr, gm = _same_groups(pos, mot, 4, off, ln, m)
    assert np.diff(gf)[gm == 1].tolist() == [4096, 4096, 1, 4096, 4096, 3, 3] and gr[gm == 1].tolist() == [0, 1, 1, 2, 2, 2, 3]
    assert gm.tolist() == sorted(gm.tolist()) and set(gm.tolist()) == {1, 2}
    assert int(gf[np.searchsorted(gm, 2)]) == win.size                  # motif 2's groups are anchored at ITS first hit


def test_groups_reject_what_the_definition_excludes_and_the_capacity_protocol():
    off, ln = _table([20, 30, 10])
    good = (np.asarray([0, 5, 21, 3, 40]), np.asarray([0, 0, 0, 2, 2], dtype=np.int32))
    _same_groups(good[0], good[1], 3, off, ln, 4)

    def refused(pos, mot, n_motifs=3, off=off, ln=ln, m=4):
        with pytest.raises(ValueError):
            _lib.site_groups_lib(np.asarray(pos), np.asarray(mot, dtype=np.int32), n_motifs, off, ln, m)
        with pytest.raises(ValueError):
            lrules.groups(pos, mot, n_motifs, off, ln, m)

    refused([0, 5, 21, 3, 40], [0, 0, 2, 1, 2])              # motifs descend
    refused([0, 5, 21, 3, 40], [0, 0, 0, 2, 3])              # no motif of the library
    refused([0, 5, 21, 3, 40], [-1, 0, 0, 2, 2])
    refused([0, 5, 5, 3, 40], [0, 0, 0, 2, 2])               # not strictly ascending inside a motif
    refused([5, 0, 21, 3, 40], [0, 0, 0, 2, 2])
    refused([0, 17, 21, 3, 40], [0, 0, 0, 2, 2])             # a window crosses its record's end
    refused([0, 5, 20, 3, 40], [0, 0, 0, 2, 2])              # a hit on a separator
    refused([0, 5, 21, 3, 70], [0, 0, 0, 2, 2])              # past the stream
    refused([0, 5, 21, 3, 40], [0, 0, 0, 2, 2], m=0)
    refused([0, 5, 21, 3, 40], [0, 0, 0, 2, 2], off=np.asarray([0, 20, 52]))      # a record on its neighbour's separator
    refused([0, 5, 21, 3, 40], [0, 0, 0, 2, 2], ln=np.asarray([20, -1, 10]))
    with pytest.raises(ValueError):
        _lib.site_order_lib(good[0], np.asarray([0, 0, 0, 2, 3], dtype=np.int32), 3)
    with pytest.raises(ValueError):
        _lib.site_order_lib(good[0], np.asarray([0, 0, -1, 2, 2], dtype=np.int32), 3)
    # the capacity protocol, on the C ABI itself
    L = _lib.load()
    pos, mot = np.ascontiguousarray(good[0], dtype=np.int64), good[1]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                         # noqa: E731
    n = ctypes.c_int64(-1)
    first, rec, motif = np.full(5, -7, dtype=np.int64), np.full(4, -7, dtype=np.int64), np.full(4, -7, dtype=np.int64)
    args = (p(pos), p(mot), 5, 3, p(off), p(ln), 3, 4)
    for cap in (0, 3):
        assert L.pfmscan_site_groups_lib(*args, cap, p(first), p(rec), p(motif), ctypes.byref(n)) == _lib.E_CAPACITY
        assert n.value == 4 and (first == -7).all() and (rec == -7).all() and (motif == -7).all()      # nothing was written
    assert L.pfmscan_site_groups_lib(*args, 4, p(first), p(rec), p(motif), ctypes.byref(n)) == 0 and n.value == 4
    assert first.tolist() == [0, 2, 3, 4, 5] and rec.tolist() == [0, 1, 0, 1] and motif.tolist() == [0, 0, 2, 2]
    assert L.pfmscan_site_groups_lib(p(pos), p(mot), 0, 3, p(off), p(ln), 3, 4, 0, p(first), None, None, ctypes.byref(n)) == 0
    assert n.value == 0 and first[0] == 0


def test_the_library_exports_the_new_entry_points():
    L = _lib.load()
    for name in ("pfmscan_site_groups_lib", "pfmscan_site_order_lib", "pfmscan_site_acc_add", "pfmscan_site_acc_round",
                 "pfmscan_site_acc_from_doubles", "pfmscan_site_sums_lib_dev", "pfmscan_site_sums_lib_staged"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    assert _lib.ABI_VERSION >= 16 and L.pfmscan_abi_version() == _lib.ABI_VERSION and _lib.SITE_LIMBS == lrules.LIMBS == 66
    header = open(os.path.join(REPO, "include", "pfmscan.h")).read()
    assert "#define PFMSCAN_SITE_LIMBS 66" in header


# ---- 4. the rules engine's accumulators are the restated sums --------------------------------------------------------------
def test_the_rules_engine_equals_per_motif_fsum_of_the_group_rows():
    from rnascan_amd import pack
    rng = np.random.default_rng(4)
    m, flank, n_motifs = 5, 2, 3
    profs = [rng.random((L, 7)) * rng.choice([1e-300, 1.0, 1e300], size=(L, 7)) for L in (30, 5, 44)]
    codes = [rng.integers(0, 6, size=L).astype(np.uint8) for L in (30, 5, 44)]
    st = pack.pack(code_arrays=codes, profiles=profs, profile_dtype=np.float64)
    win = np.flatnonzero(st.window_mask(m)).astype(np.int64)
    pos = np.concatenate([win[::2], win[1::3]])
    mot = np.concatenate([np.zeros(win[::2].size, np.int32), np.full(win[1::3].size, 2, np.int32)])
    order = np.lexsort((mot, pos))
    acc, counts = RulesEngine().site_sums_library(st, pos[order], mot[order], n_motifs, m, flank)
    assert lrules.normalised(acc) and not acc[1].any() and not counts[1].any()
    S = _lib.site_acc_round(acc).reshape(n_motifs, m + 2 * flank, 7)
    for k in (0, 2):
        _, rows, cnt = rules.site_sums(st.profile, st.codes, pos[mot == k], st.offsets, st.lengths, m, flank)
        assert np.array_equal(bits(S[k]), bits(rules.total(rows))) and np.array_equal(counts[k], cnt.sum(axis=0))


# ---- 5. the command --------------------------------------------------------------------------------------------------------
def _run(argv, engine=None):
    prefix = argv[argv.index("-o") + 1]
    rc = sites.main(list(argv), engine=engine or RulesEngine())
    out = {}
    for ext in (".struct.txt", ".seq.txt", ".counts.txt"):
        if os.path.exists(prefix + ext):
            out[ext] = open(prefix + ext, "rb").read()
    return rc, out


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sites_lib")
    fa, avg, sdir = helpers.sites_helpers.write_inputs(tmp)
    lib_seq, lib_struct, pairs = helpers.write_library(tmp)
    return tmp, fa, avg, sdir, lib_seq, lib_struct, pairs


MODES = {
    "both": (["-C", "0.05", "-m", "-25"], True, True),
    "seq": (["-m", "4"], True, False),
    "struct": (["-C", "0.05", "-m", "-14"], False, True),
    "seqstruct": (["-C", "0.05", "-m", "-25", "--min-seqstruct", "-18"], True, True),
    "flank": (["-C", "0.05", "-m", "-25", "--min-seqstruct", "-18", "--flank", "5"], True, True),
}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_all_motifs_equals_one_single_motif_run_per_pair_byte_for_byte(inputs, mode, tmp_path, capfd):
    _, fa, avg, sdir, lib_seq, lib_struct, pairs = inputs
    opts, use_seq, use_struct = MODES[mode]
    tail = opts + ([fa] if use_seq else []) + [avg]
    argv = ["--all-motifs", "-o", str(tmp_path / "all")] + (["-p", lib_seq] if use_seq else []) + (["-q", lib_struct] if use_struct else []) + tail
    rc, got = _run(argv)
    err = capfd.readouterr().err
    want = helpers.assemble_single_runs(tmp_path, pairs, tail, RulesEngine(), use_seq, use_struct, flank=5 if mode == "flank" else 0)
    assert rc == 0 and sorted(got) == sorted(k for k, v in want.items() if v)
    for ext in got:
        assert got[ext] == want[ext], (mode, ext)
    assert got[".struct.txt"].count(b"#PO") >= 2 and (b"#SLBP\n" in got[".struct.txt"])
    assert got[".counts.txt"].startswith(b"Motif\tPO\tSites\tCoverage")
    for name, _, _ in pairs:                                # every motif has its counts block; the ones left out are named
        assert (b"\n" + name.encode() + b"\t0\t") in got[".counts.txt"]
        if (b"#" + name.encode() + b"\n") not in got[".struct.txt"]:
            assert "Motif %s:" % name in err
    if mode in ("both", "seqstruct", "struct"):
        # the multi-PFM output loads as a library, and of the widths that went in
        lib = cli.load_motif(str(tmp_path / "all.struct.txt"), 0.01, fasta.STRUCT, None)
        assert set(v.length for v in lib.values()) <= {18, 12} and len(lib) == got[".struct.txt"].count(b"#PO")
    if use_seq:
        lib = cli.load_motif(str(tmp_path / "all.seq.txt"), 0.01, fasta.RNA, None)
        assert len(lib) == got[".seq.txt"].count(b"#PO")


def test_all_motifs_does_not_depend_on_batches_input_form_record_order_or_ranks(inputs, tmp_path, monkeypatch):
    _, fa, avg, sdir, lib_seq, lib_struct, _ = inputs
    opts = ["--all-motifs", "-p", lib_seq, "-q", lib_struct, "-C", "0.05", "-m", "-25", "--min-seqstruct", "-18", "--flank", "2"]
    rc, one = _run(opts + ["-o", str(tmp_path / "one"), fa, avg])
    assert rc == 0 and len(one) == 3
    for batch in ("1", "300", "2000"):
        monkeypatch.setenv("RNASCAN_BATCH_POSITIONS", batch)
        assert _run(opts + ["-o", str(tmp_path / ("b" + batch)), fa, avg]) == (0, one)
    assert _run(opts + ["-o", str(tmp_path / "store"), fa, sdir]) == (0, one)
    monkeypatch.delenv("RNASCAN_BATCH_POSITIONS")
    recs = list(fasta.open_lazy(fa))
    other = str(tmp_path / "reversed.fa")
    write_fasta(other, [(r.id, r.seq) for r in reversed(recs)])
    assert _run(opts + ["-o", str(tmp_path / "rev"), other, sdir]) == (0, one)
    # ranks: the accumulators of every rank, added, are the accumulators of one
    args = sites.getoptions(opts + ["-o", str(tmp_path / "r"), fa, sdir])
    seq = cli.load_motif(args.pfm_seq, args.pseudocount, fasta.RNA, None)
    st = cli.load_motif(args.pfm_struct, args.pseudocount, fasta.STRUCT, None)

    def same(a, b):
        return len(a) == len(b) and all(x[0] == y[0] and np.array_equal(bits(x[1]), bits(y[1])) and np.array_equal(x[2], y[2]) and
                                        np.array_equal(x[3], y[3]) and x[4] == y[4] for x, y in zip(a, b))
    single = sites.gather_library(RulesEngine(), args, seq, st)
    for world in (1, 2):
        got = as_ranks(world, lambda r, w, dist: sites.gather_library(RulesEngine(), args, seq, st, r, w, dist))
        assert all(isinstance(g, list) and same(g, single) for g in got), got


def test_a_motif_without_sites_is_named_and_skipped_and_none_at_all_is_exit_1(inputs, tmp_path, capfd):
    _, fa, avg, sdir, lib_seq, _, pairs = inputs
    # a sequence motif that no record holds: sixteen Cs then two Gs, never in the random records at this threshold
    never = np.full((18, 4), 0.001)
    never[:16, 1] = never[16:, 2] = 0.997
    tmp2 = tmp_path / "lib2"
    tmp2.mkdir()
    lib2, _, _ = helpers.write_library(tmp2, extra=[("never", never, np.full((18, 7), 1 / 7.0))])
    rc, got = _run(["--all-motifs", "-p", lib2, "-m", "12", "-o", str(tmp_path / "x"), fa, sdir])
    err = capfd.readouterr().err
    assert rc == 0 and b"#SLBP\n" in got[".struct.txt"] and b"#never\n" not in got[".struct.txt"]
    assert "Motif never: no site" in err
    rows = [ln.split(b"\t") for ln in got[".counts.txt"].splitlines() if ln.startswith(b"never\t")]
    assert len(rows) == 18 and all(r[2] == b"0" and r[3] == b"0" for r in rows)
    only = str(tmp_path / "only.txt")
    helpers._write_multi(only, [("never", never), ("never2", never)], list("ACGU"))
    rc, got = _run(["--all-motifs", "-p", only, "-m", "12", "-o", str(tmp_path / "y"), fa, sdir])
    assert rc == 1 and got == {}
    assert "no files written" in capfd.readouterr().err


def test_accumulators_beyond_the_limit_name_the_flank(inputs, tmp_path, capfd, monkeypatch):
    """2 GiB takes 256 motifs at W > 2200; the check itself is exercised with the limit lowered to the two 18-wide motifs'
    accumulators at --flank 3 less one byte"""
    _, fa, avg, sdir, lib_seq, _, _ = inputs
    assert sites.ACC_LIMIT == 1 << 31 and 256 * 2300 * 7 * 66 * 8 > sites.ACC_LIMIT
    monkeypatch.setattr(sites, "ACC_LIMIT", 2 * (18 + 2 * 3) * 7 * 66 * 8 - 1)
    rc, got = _run(["--all-motifs", "-p", lib_seq, "-m", "4", "--flank", "3", "-o", str(tmp_path / "z"), fa, sdir])
    assert rc == 1 and got == {} and "--flank" in capfd.readouterr().err


def test_without_the_flag_a_library_file_still_means_its_first_motif(inputs, tmp_path):
    _, fa, avg, sdir, lib_seq, lib_struct, pairs = inputs
    first = [p for p in pairs if p[0] == "SLBP"][0]              # the first block of the library files
    tail = ["-C", "0.05", "-m", "-25", "--min-seqstruct", "-18", fa, sdir]
    a = _run(["-p", lib_seq, "-q", lib_struct, "-o", str(tmp_path / "a")] + tail)
    b = _run(["-p", first[1], "-q", first[2], "-o", str(tmp_path / "b")] + tail)
    assert a[0] == 0 and a == b and not a[1][".struct.txt"].startswith(b"#")


# ---- 6. the host-only native code under the sanitizers ---------------------------------------------------------------------
def test_sites_lib_host_under_sanitizers(tmp_path):
    """pfmscan_sites_lib_host.hip has no device code: compiled with g++ -fsanitize=address,undefined beside a stand-alone
    driver (tests/c/fuzz_sites_lib.cpp, its own main) that feeds it random and adversarial lists in exact-size heap buffers"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "fuzz_sites_lib")
    csrc = os.path.join(REPO, "rnascan_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tests", "c", "fuzz_sites_lib.cpp"),
           "-x", "c++", os.path.join(csrc, "pfmscan_sites_lib_host.hip"), os.path.join(csrc, "pfmscan_sites_host.hip"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().startswith("ok"), (run.stdout + run.stderr)[-3000:]
