"""Site profiles of a motif library on the device (pfmscan_site_sums_lib_*): the long accumulators against the exact
Python-int sums of the restated group values (tests/sites_lib_rules.py), LIMB-EXACT, the rounded sums against math.fsum
over the group rows the single-motif entry point returns, bit for bit; both entry-point forms; rejections; broken tables."""
import math

import numpy as np
import pytest

import sites_lib_rules as lrules
import sites_rules as rules

pytestmark = pytest.mark.gpu

BIG = 2e306            # its pieces reach limb 65; 800 of them still sum below DBL_MAX


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make_stream(rng, lengths, dtype, wide=True):
    """rows whose cells are spread over the exponent range of their format (subnormals included), a few zeros, and codes
    with foreign letters inside the records"""
    from rnascan_amd import pack
    profs, codes = [], []
    for L in lengths:
        p = rng.random((L, 7)) + 0.5
        if dtype == np.float64:
            scale = rng.choice([5e-324, 1e-300, 1.0, 1e300, BIG] if wide else [1e-300, 1.0, 1e-7], size=(L, 7),
                               p=[.2, .2, .4, .197, .003] if wide else [.3, .4, .3])
            p = np.where(scale == 5e-324, rng.integers(1, 9, size=(L, 7)) * 5e-324, p * scale)
        else:
            tiny = float(np.finfo(np.float32).smallest_subnormal)
            scale = rng.choice([tiny, 1e-38, 1.0, 1e35] if wide else [1e-38, 1.0, 1e-7], size=(L, 7), p=[.2, .2, .4, .2] if wide else [.3, .4, .3])
            p = np.where(scale == tiny, rng.integers(1, 9, size=(L, 7)) * tiny, p * scale)
        p[rng.random((L, 7)) < 0.05] = 0.0
        if wide and dtype == np.float64 and L > 0 and not profs:
            p[0, :2] = 5e-324, BIG                      # under the first record's first window: limbs 0 and 65 are written
        profs.append(p.astype(dtype))
        codes.append(rng.choice(np.arange(8, dtype=np.uint8), size=L, p=[.22, .22, .22, .22, .03, .03, .03, .03]))
    return pack.pack(code_arrays=codes, profiles=profs, profile_dtype=dtype)


def library_hits(rng, st, m, n_motifs, empty=(), density=0.3):
    """(pos, motif) in (position, motif) order, as the library scans return hits; the motifs in ``empty`` have none"""
    win = np.flatnonzero(st.window_mask(m)).astype(np.int64)
    pos, mot = [], []
    for k in range(n_motifs):
        if k in empty:
            continue
        keep = rng.random(win.size) < density
        keep[0] = keep[-1] = True
        keep[np.searchsorted(win, st.offsets[st.lengths >= m])] = True       # every record's first window
        pos.append(win[keep])
        mot.append(np.full(int(keep.sum()), k, dtype=np.int32))
    pos, mot = np.concatenate(pos), np.concatenate(mot)
    order = np.lexsort((mot, pos))
    return pos[order], mot[order]


def dev_form(ctx, st, pos, mot, n_motifs, m, flank, tables=None, use_codes=True):
    """pfmscan_site_sums_lib_dev on torch buffers, motif-major (pos, mot) -> (raw acc, counts)"""
    import torch
    dev = torch.device("cuda", 0)
    gf, gr, gm = tables if tables is not None else lrules.groups(pos, mot, n_motifs, st.offsets, st.lengths, m)
    W = m + 2 * flank
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)            # noqa: E731
    prof, codes, d_pos = up(st.profile), up(st.codes), up(np.asarray(pos, dtype=np.int64))
    d_gf, d_gr, d_gm, off, ln = up(gf), up(gr), up(gm), up(st.offsets), up(st.lengths)
    acc = torch.full((n_motifs, lrules.LIMBS, W * 7), -1, dtype=torch.int64, device=dev)       # the call zeroes them itself
    counts = torch.full((n_motifs, W, 8), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.site_sums_lib_dev(codes.data_ptr() if use_codes else None, prof.data_ptr(), st.profile.dtype, st.profile.shape[0],
                          d_pos.data_ptr(), len(pos), d_gf.data_ptr(), d_gr.data_ptr(), d_gm.data_ptr(), len(gr), off.data_ptr(),
                          ln.data_ptr(), len(st.offsets), n_motifs, m, flank, acc.data_ptr(), counts.data_ptr() if use_codes else None)
    ctx.synchronize()
    torch.cuda.synchronize()
    return acc.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint64)


def fsum_rows(rows):
    out = np.zeros(rows.shape[1:], dtype=np.float64)
    flat, o = rows.reshape(rows.shape[0], out.size), out.reshape(-1)
    for e in range(o.size):
        try:
            o[e] = math.fsum(flat[:, e].tolist())
        except OverflowError:
            o[e] = np.inf
    return out


def check(engine, st, pos, mot, n_motifs, m, flank):
    from rnascan_amd import _lib
    ctx = engine.ctx
    W = m + 2 * flank
    A, counts, _ = lrules.site_sums_library(st.profile, st.codes, pos, mot, n_motifs, st.offsets, st.lengths, m, flank)
    ctx.stage(st.codes, st.profile)
    acc, cnt = ctx.site_sums_lib_staged(pos, mot, n_motifs, st.offsets, st.lengths, m, flank)
    assert acc.shape == (n_motifs, lrules.LIMBS, W * 7) and lrules.normalised(acc)
    got = lrules.acc_int(acc)
    assert np.array_equal(got, A), (m, flank, np.argwhere(got != A)[:5])
    assert np.array_equal(cnt.astype(np.int64), counts)
    # rounded == math.fsum over the group rows of the single-motif entry point, per motif
    S = _lib.site_acc_round(acc).reshape(n_motifs, W, 7)
    for k in range(n_motifs):
        _, rows, gcnt = ctx.site_sums_staged(pos[mot == k], st.offsets, st.lengths, m, flank)
        assert np.array_equal(bits(S[k]), bits(fsum_rows(rows))), (k, m, flank)
        assert np.array_equal(cnt[k].astype(np.int64), gcnt.astype(np.int64).sum(axis=0))
    # the _dev form: raw limbs, the same integers; twice, the same limbs
    order = lrules.motif_major(pos, mot)
    raw, dcnt = dev_form(ctx, st, pos[order], mot[order], n_motifs, m, flank)
    assert np.array_equal(lrules.acc_int(raw), A)
    assert np.array_equal(dcnt, cnt)
    assert np.array_equal(_lib.site_acc_add(np.zeros_like(raw), raw), acc)
    again, _ = dev_form(ctx, st, pos[order], mot[order], n_motifs, m, flank)
    assert np.array_equal(again, raw)
    return acc, cnt


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m,flank,n_motifs,empty", [(1, 0, 1, ()), (1, 3, 3, (0,)), (9, 0, 2, ()), (10, 0, 3, (2,)), (10, 3, 4, (0, 3)),
                                                    (10, 15, 5, (0, 4)), (9, 3, 2, ())])
def test_limbs_equal_the_exact_integer_sums(engine, m, flank, n_motifs, empty, dtype):
    """7, 63 and 70 cells (the second 64-cell walk), W = 40 (280 cells); a record exactly m long (the flanks hang over
    both ends), records shorter than m, foreign letters inside records; empty motifs first and last"""
    rng = np.random.default_rng(1000 * m + 10 * flank + n_motifs)
    lengths = [m, m + 1, 3, m + 37, 2 * m + 5, m, 0, m + 101, m + 11]
    st = make_stream(rng, lengths, dtype)
    pos, mot = library_hits(rng, st, m, n_motifs, empty)
    acc, _ = check(engine, st, pos, mot, n_motifs, m, flank)
    for k in empty:
        assert not acc[k].any()
    if dtype == np.float64 and m >= 9:
        assert acc[:, 0].any() and acc[:, lrules.LIMBS - 1].any()         # the first and the last limb are written


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_groups_of_every_size(engine, dtype):
    """(motif, record) runs of 1, 3, 4, 5, 8, 9, 4096 and 4097 hits: every remainder of the unrolled-by-four walk, a full
    group, and a full group with a group of one behind it"""
    rng = np.random.default_rng(11)
    m = 12
    sizes = [1, 3, 4, 5, 8, 9, 4096, 4097]
    st = make_stream(rng, [n + m - 1 for n in sizes], dtype, wide=False)
    win = np.flatnonzero(st.window_mask(m)).astype(np.int64)
    thin = win[rng.random(win.size) < 0.4]
    pos = np.concatenate([win, thin])
    mot = np.concatenate([np.full(win.size, 1, dtype=np.int32), np.full(thin.size, 2, dtype=np.int32)])
    order = np.lexsort((mot, pos))
    pos, mot = pos[order], mot[order]
    gf, _, gm = lrules.groups(pos[lrules.motif_major(pos, mot)], np.sort(mot), 4, st.offsets, st.lengths, m)
    assert sorted(np.diff(gf)[gm == 1].tolist()) == sorted([1, 3, 4, 5, 8, 9, 4096, 4096, 1])
    check(engine, st, pos, mot, 4, m, 0)


def test_two_batches_merged_equal_one(engine):
    from rnascan_amd import _lib, pack
    rng = np.random.default_rng(5)
    m, flank, n_motifs = 10, 3, 3
    lengths = [40, m, 77, 0, 55, 91, 33]
    st = make_stream(rng, lengths, np.float64)
    pos, mot = library_hits(rng, st, m, n_motifs)
    ctx = engine.ctx
    ctx.stage(st.codes, st.profile)
    whole, wcnt = ctx.site_sums_lib_staged(pos, mot, n_motifs, st.offsets, st.lengths, m, flank)
    cut = 3
    total = np.zeros_like(whole)
    tcnt = np.zeros_like(wcnt)
    for a, b in ((0, cut), (cut, len(lengths))):
        lo, hi = int(st.offsets[a]), int(st.offsets[b - 1] + st.lengths[b - 1])
        part = pack.Stream(st.codes[lo:hi + 1].copy(), st.profile[lo:hi + 1].copy(), st.offsets[a:b] - lo, st.lengths[a:b])
        keep = (pos >= lo) & (pos < hi)
        ctx.stage(part.codes, part.profile)
        acc, cnt = ctx.site_sums_lib_staged(pos[keep] - lo, mot[keep], n_motifs, part.offsets, part.lengths, m, flank)
        _lib.site_acc_add(total, acc)
        assert lrules.normalised(total)
        tcnt += cnt
    assert np.array_equal(total, whole) and np.array_equal(tcnt, wcnt)


# ---- rejections ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf, -1.0])
def test_bad_cell_under_one_motifs_hit_is_rejected_smallest_index_first(engine, value):
    rng = np.random.default_rng(3)
    m, flank, n_motifs = 9, 3, 3
    st = make_stream(rng, [60, 80, 70], np.float64, wide=False)
    pos = np.asarray([5, 30, 70, 100, 150, 170], dtype=np.int64)
    mot = np.asarray([0, 1, 0, 2, 1, 0], dtype=np.int32)
    order = np.lexsort((mot, pos))
    pos, mot = pos[order], mot[order]
    ctx = engine.ctx
    prof = st.profile.copy()
    prof[50, 2] = value                               # under no hit (30 + 9 + 3 = 42 is the last column of the hit at 30)
    ctx.stage(st.codes, prof)
    ctx.site_sums_lib_staged(pos, mot, n_motifs, st.offsets, st.lengths, m, flank)
    prof[105, 4] = value                              # under the hit of motif 2 at 100 only
    prof[152, 1] = value                              # ... and a later one under motif 1's
    ctx.stage(st.codes, prof)
    with pytest.raises(ValueError) as e:
        ctx.site_sums_lib_staged(pos, mot, n_motifs, st.offsets, st.lengths, m, flank)
    assert e.value.element == 105 * 7 + 4 == rules.first_bad(prof, pos, st.offsets, st.lengths, m, flank)
    # a flank column that hangs over the record end is skipped: a bad cell in the separator row is no error
    prof = st.profile.copy()
    prof[60, 0] = value
    ctx.stage(st.codes, prof)
    ctx.site_sums_lib_staged(np.asarray([51], dtype=np.int64), np.asarray([1], dtype=np.int32), n_motifs, st.offsets, st.lengths, m, flank)


def test_group_cell_that_overflows_from_finite_cells_is_rejected(engine):
    rng = np.random.default_rng(4)
    st = make_stream(rng, [30], np.float64, wide=False)
    prof = st.profile.copy()
    prof[10, 3] = prof[11, 3] = 1.5e308
    engine.ctx.stage(st.codes, prof)
    with pytest.raises(ValueError, match="overflow") as e:
        engine.ctx.site_sums_lib_staged(np.asarray([10, 11], dtype=np.int64), np.zeros(2, dtype=np.int32), 1, st.offsets, st.lengths, 1, 0)
    assert getattr(e.value, "element", None) is None
    acc, _ = engine.ctx.site_sums_lib_staged(np.asarray([10], dtype=np.int64), np.zeros(1, dtype=np.int32), 1, st.offsets, st.lengths, 1, 0)
    assert lrules.acc_int(acc)[0, 3] == lrules.as_int(1.5e308)


def test_broken_tables_are_rejected_on_the_device(engine):
    rng = np.random.default_rng(6)
    m, n_motifs = 4, 3
    st = make_stream(rng, [50, 4200, 60], np.float64, wide=False)
    ctx = engine.ctx
    pos = np.asarray([3, 20, 60, 4300, 10, 70], dtype=np.int64)
    mot = np.asarray([0, 0, 0, 0, 2, 2], dtype=np.int64)
    gf, gr, gm = lrules.groups(pos, mot, n_motifs, st.offsets, st.lengths, m)
    dev_form(ctx, st, pos, mot, n_motifs, m, 1, (gf, gr, gm))              # the table itself is fine

    def broken(p=pos, f=gf, r=gr, k=gm):
        with pytest.raises(ValueError) as e:
            dev_form(ctx, st, p, mot, n_motifs, m, 1, (np.asarray(f), np.asarray(r), np.asarray(k)))
        assert getattr(e.value, "element", None) is None

    broken(k=gm[::-1].copy())                                             # grp_motif descends
    broken(k=np.where(gm == 2, n_motifs, gm))                             # no motif of the library
    broken(k=np.where(gm == 0, -1, gm))
    broken(p=np.asarray([3, 20, 60, 4300, 70, 10], dtype=np.int64))       # positions descend inside motif 2
    broken(p=np.asarray([3, 3, 60, 4300, 10, 70], dtype=np.int64))        # ... do not ascend strictly
    broken(p=np.asarray([3, 47, 60, 4300, 10, 70], dtype=np.int64))       # a window leaves its record
    broken(r=np.where(np.arange(gr.size) == 0, 1, gr))                    # a hit outside the record of its group
    broken(f=gf[:-1].tolist() + [pos.size - 1])                           # the groups do not cover the hits
    broken(r=np.where(np.arange(gr.size) == 0, 7, gr))                    # no record
    # a group of 4097 hits of one (motif, record)
    dense = np.arange(51, 51 + 4097, dtype=np.int64)
    zeros = np.zeros(dense.size, dtype=np.int64)
    with pytest.raises(ValueError) as e:
        dev_form(ctx, st, dense, zeros, n_motifs, m, 0, (np.asarray([0, 4097]), np.asarray([1]), np.asarray([0])))
    assert getattr(e.value, "element", None) is None
    dev_form(ctx, st, dense, zeros, n_motifs, m, 0)                       # cut properly it is taken


# ---- the command -------------------------------------------------------------------------------------------------------
def test_all_motifs_command_equals_the_rules_engine_and_the_single_motif_runs(engine, tmp_path, capsys):
    """a width group of two pairs at a finite -m goes through the library kernels' hits; the GPU files equal the rules
    engine's byte for byte, and each motif's block the files of the existing single-motif command"""
    import sites_lib_helpers as helpers
    from rnascan_amd import sites
    fa, avg, lib_seq, lib_struct, pairs = helpers.write_library_inputs(tmp_path)
    tail = ["-C", "0.05", "-m", "-25", "--min-seqstruct", "-18", fa, avg]
    common = ["-p", lib_seq, "-q", lib_struct] + tail
    assert sites.main(["--all-motifs", "-o", str(tmp_path / "gpu")] + common, engine=engine) == 0
    assert sites.main(["--all-motifs", "-o", str(tmp_path / "cpu")] + common, engine=helpers.RulesEngine()) == 0
    for ext in (".struct.txt", ".seq.txt", ".counts.txt"):
        assert (tmp_path / ("gpu" + ext)).read_bytes() == (tmp_path / ("cpu" + ext)).read_bytes(), ext
    want = helpers.assemble_single_runs(tmp_path, pairs, tail, engine)
    for ext in (".struct.txt", ".seq.txt", ".counts.txt"):
        assert (tmp_path / ("gpu" + ext)).read_bytes() == want[ext], ext
