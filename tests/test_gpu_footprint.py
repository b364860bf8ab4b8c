"""The posterior site map (k_fp_tiles, csrc/pfmscan_footprint.hip) on the GPU against the rules (tests/footprint_rules.py):
every comparison is on the float64 bit patterns (NaN == NaN), the int64 keys and Windows -- there is no tolerance in the
contract."""
import ctypes

import numpy as np
import pytest

import expect_rules as erules
import footprint_rules as rules
import occupancy_rules as orules
import pair_rules as prules

pytestmark = pytest.mark.gpu

MODES = (rules.RATIO, rules.POSTERIOR)
SENTINEL = np.array([0x7FF8DEAD0000BEEF], dtype=np.uint64).view(np.float64)[0]   # a NaN with a payload nothing computes


def tile_of(m):
    from rnascan_amd import _lib
    return _lib.FOOTPRINT_SLOTS - (m - 1)


def stage(ctx, codes, codes2):
    ctx.stage(codes if codes is not None else codes2)
    if codes2 is not None:
        ctx.stage_codes2(codes2)


def run(ctx, codes, codes2, off, lens, R, S, mode, **kw):
    stage(ctx, codes, codes2)
    return ctx.footprint_staged(R, S, mode, off, lens, **kw)


def same(got, want):
    return (rules.same_bits(got[0], want[0]) and rules.same_bits(got[1], want[1]) and rules.same_bits(got[2], want[2]) and
            got[3].dtype == np.int64 and np.array_equal(got[3], want[3]))


def check(ctx, codes, codes2, off, lens, R, S, mode):
    got = run(ctx, codes, codes2, off, lens, R, S, mode)
    want = rules.footprint(codes, codes2, off, lens, R, S, mode)
    for name, g, w in zip(("start", "cover", "occ"), got, want):
        assert rules.same_bits(g, w), "%s bits differ at %s" % (name, np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])
    assert got[3].dtype == np.int64 and np.array_equal(got[3], want[3])
    return got


def ladder(rng, m):
    """every length 0 .. 3 m + 2, the lengths around the kernel's tile (as windows and as positions), short records in between"""
    tile = tile_of(m)
    around = [n + m - 1 for n in (tile - 1, tile, tile + 1, 2 * tile + 1)] + [tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1]
    lengths = list(range(0, 3 * m + 3))
    for x in around:
        lengths += [x, int(rng.integers(0, 2 * m + 2))]
    return lengths


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [1, 2, 8, 12, 33, 64])
def test_length_ladder(ctx, m, mode):
    rng = np.random.default_rng(500 + 2 * m + mode)
    lengths = ladder(rng, m)
    codes, off, lens = rules.stream(rng, lengths, 4, foreign=0.002)
    n_win, tile = np.maximum(lens - m + 1, 0), tile_of(m)
    for n in (tile - 1, tile, tile + 1, 2 * tile + 1):
        assert (n_win == n).any() and (lens == n).any()
    for L in range(0, 3 * m + 3):
        assert (lens == L).any()
    R = rules.table(rng, m, 4, 0.6, 1.7)
    start, cover, occ, win = check(ctx, codes, None, off, lens, R, None, mode)
    assert not np.signbit(start).any() and not np.signbit(cover).any() and np.isfinite(cover).all()
    for o, n in zip(off, lens):                                    # the record's last min(m - 1, L) starts, and the separator behind it
        assert (start[0, o + max(n - m + 1, 0):o + n + 1] == 0).all() and cover[0, o + n] == 0
    if mode == rules.POSTERIOR:
        for o, n, nw in zip(off, lens, n_win):
            if nw > 0:
                assert cover[0, o:o + n].max() <= rules.cover_bound(int(nw), m)
    o2, w2 = ctx.occupancy_staged(R, 4, off, lens, 0)
    assert rules.same_bits(o2, occ) and np.array_equal(w2, win)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [1, 8, 21])
def test_foreign_codes(ctx, m, mode):
    rng = np.random.default_rng(13 * m + mode)
    L = 2 * m + 37
    codes, off, lens = rules.stream(rng, [L] * (L + 1) + [3 * m + 150, tile_of(m) + 3 * m])
    for p in range(L):                                             # record p: one foreign code at position p (every offset of a window)
        codes[off[p] + p] = np.uint8(rng.integers(4, 8))
    codes[off[L]:off[L] + L] = 7                                   # a record of nothing else
    codes[off[-2] + 60] = codes[off[-2] + 60 + max(m - 1, 1)] = 5  # two within m
    t = tile_of(m)
    codes[off[-1] + t - 1] = codes[off[-1] + t + m - 1] = 6        # on either side of a tile's edge
    R = rules.table(rng, m, 4)
    start, cover, occ, win = check(ctx, codes, None, off, lens, R, None, mode)
    assert win[L] == 0 and occ[L, 0] == 0 and (start[0, off[L]:off[L] + L] == 0).all() and (cover[0, off[L]:off[L] + L] == 0).all()
    assert win[0] == L - m and win[L - 1] == L - m


@pytest.mark.parametrize("mode", MODES)
def test_structure_letters_from_codes2(ctx, mode):
    rng = np.random.default_rng(41 + mode)
    m = 9
    codes2, off, lens = rules.stream(rng, [int(x) for x in rng.integers(0, 900, size=40)] + [2 * tile_of(m) + 5], 7, foreign=0.003, case=True)
    assert (codes2 & 8).any()
    S = rules.table(rng, m, 7, 0.6, 1.7)
    got = check(ctx, None, codes2, off, lens, None, S, mode)
    plain = codes2.copy()
    plain[plain != 7] &= 7
    assert same(run(ctx, None, plain, off, lens, None, S, mode), got)
    # codes that are staged beside them are not read
    noise = rng.integers(0, 8, size=codes2.size).astype(np.uint8)
    assert same(run(ctx, noise, codes2, off, lens, None, S, mode), got)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [1, 8, 21])
def test_pairs_with_a_foreign_code_in_either_stream(ctx, m, mode):
    rng = np.random.default_rng(7 * m + mode)
    L = 2 * m + 19
    codes, codes2, off, lens = prules.streams(rng, [L] * (2 * L) + [tile_of(m) + 2 * m, 0, 3], case=True)
    for p in range(L):
        codes[off[p] + p] = np.uint8(rng.integers(4, 8))
        codes2[off[L + p] + p] = np.uint8(7 | (8 if rng.random() < 0.3 else 0))
    codes2[off[-3] + tile_of(m)] = 7
    R, S = rules.table(rng, m, 4), rules.table(rng, m, 7)
    got = check(ctx, codes, codes2, off, lens, R, S, mode)
    o2, w2 = ctx.occupancy_pair_staged(R, S, off, lens)
    assert rules.same_bits(o2, got[2]) and np.array_equal(w2, got[3])


@pytest.mark.parametrize("mode", MODES)
def test_the_two_identities_against_the_single_stream_calls(ctx, mode):
    rng = np.random.default_rng(19 + mode)
    for m in (8, 21):
        lengths = [int(x) + m - 1 for x in rng.integers(1, 900, size=20)] + [m - 1, 1300]
        Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(2)])
        Ss = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(2)])
        one = np.stack([prules.ones(m)] * 2)
        codes, codes2, off, lens = prules.streams(rng, lengths, foreign_seq=0.004, foreign_struct=0.0, case=True)
        assert same(run(ctx, codes, codes2, off, lens, Rs, one, mode), run(ctx, codes, codes2, off, lens, Rs, None, mode))
        codes, codes2, off, lens = prules.streams(rng, lengths, foreign_seq=0.0, foreign_struct=0.004, case=True)
        assert same(run(ctx, codes, codes2, off, lens, one, Ss, mode), run(ctx, codes, codes2, off, lens, None, Ss, mode))


@pytest.mark.parametrize("mode", MODES)
def test_motifs_of_one_call_equal_one_call_each(ctx, mode):
    rng = np.random.default_rng(23 + mode)
    m = 12
    codes, codes2, off, lens = prules.streams(rng, [int(x) for x in rng.integers(0, 1200, size=30)], foreign_seq=0.003, foreign_struct=0.003)
    Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(4)])
    Ss = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(4)])
    for R, S in ((Rs, None), (Rs, Ss)):
        got = check(ctx, codes, codes2, off, lens, R, S, mode)
        for q in range(4):
            one = run(ctx, codes, codes2, off, lens, R[q], None if S is None else S[q], mode)
            assert same(one, (got[0][q:q + 1], got[1][q:q + 1], got[2][:, q:q + 1], got[3]))


def dev_maps(ctx, codes, codes2, off, lens, R, S, mode, want_start=True, want_cover=True, n_rec=None):
    """the _dev form on torch tensors, the planes pre-filled with the sentinel -> (start, cover) as they lie on the device"""
    import torch
    T = np.asarray(R if R is not None else S)
    n_q = 1 if T.ndim == 2 else T.shape[0]
    n_pos = int((codes if codes is not None else codes2).size)
    d_codes = torch.from_numpy(codes).cuda() if codes is not None else None
    d_codes2 = torch.from_numpy(codes2).cuda() if codes2 is not None else None
    d_off, d_len = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).cuda(), torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int64)).cuda()
    d_start = torch.from_numpy(np.full((n_q, n_pos), SENTINEL)).cuda()
    d_cover = torch.from_numpy(np.full((n_q, n_pos), SENTINEL)).cuda()
    torch.cuda.synchronize()
    ctx.footprint_dev(R, S, mode, None if d_codes is None else d_codes.data_ptr(), None if d_codes2 is None else d_codes2.data_ptr(), n_pos,
                      d_off.data_ptr(), d_len.data_ptr(), len(off) if n_rec is None else n_rec, d_start.data_ptr() if want_start else None,
                      d_cover.data_ptr() if want_cover else None)
    ctx.synchronize()
    return d_start.cpu().numpy(), d_cover.cpu().numpy()


def is_sentinel(x):
    return np.asarray(x).view(np.uint64) == SENTINEL.view(np.uint64)


def test_untouched_positions_skipped_records_and_special_tables(ctx):
    rng = np.random.default_rng(29)
    m = 8
    codes, codes2, off, lens = prules.streams(rng, [int(x) for x in rng.integers(0, 700, size=24)] + [1100], foreign_seq=0.003, foreign_struct=0.003)
    codes[off[3]:off[3] + lens[3]] = 7                             # a record without a window with a term: occ == 0
    keep = np.array([i for i in range(len(off)) if i % 3 != 1])    # a table that skips records
    tables = []
    for kind in ("plain", "zero", "inf", "nan"):
        R = rules.table(rng, m, 4)
        if kind == "zero":
            R[0, :4] = 0.0                                         # every term +0.0: every occupancy +0.0
        if kind == "inf":
            R[m - 1, 2] = np.inf
        if kind == "nan":
            R[m // 2, 0] = np.nan
        tables.append(R)
    Rs = np.stack(tables)
    S = np.stack([rules.table(rng, m, 7) for _ in tables])
    for mode in MODES:
        for R_, S_ in ((Rs, None), (Rs, S)):
            want = rules.footprint(codes, codes2, off[keep], lens[keep], R_, S_, mode, fill=SENTINEL)
            got = dev_maps(ctx, codes, codes2, off[keep], lens[keep], R_, S_, mode)
            inside = np.zeros(codes.size, dtype=bool)
            for o, n in zip(off[keep], lens[keep]):
                inside[o:o + n] = True
            for g, w in zip(got, want):
                assert is_sentinel(g[:, ~inside]).all() and not is_sentinel(g[:, inside]).any()
                assert rules.same_bits(g[:, inside], w[:, inside])
            staged = run(ctx, codes, codes2, off[keep], lens[keep], R_, S_, mode)
            zero = rules.footprint(codes, codes2, off[keep], lens[keep], R_, S_, mode)
            assert same(staged, zero) and (staged[0][:, ~inside] == 0).all() and not np.signbit(staged[1][:, ~inside]).any()
            assert (staged[0][1] == 0).all() and (staged[1][1] == 0).all() and not np.signbit(staged[1][1]).any()   # the all-zero motif
            r3 = slice(off[3], off[3] + lens[3])
            assert staged[2][list(keep).index(3), 0] == 0 and (staged[1][:, r3] == 0).all()
            assert np.isnan(staged[1][3]).any() and (np.isinf(staged[1][2]).any() or np.isnan(staged[1][2]).any())
            # one map alone: the same bits, the other plane untouched
            only_start = dev_maps(ctx, codes, codes2, off[keep], lens[keep], R_, S_, mode, want_cover=False)
            only_cover = dev_maps(ctx, codes, codes2, off[keep], lens[keep], R_, S_, mode, want_start=False)
            assert is_sentinel(only_start[1]).all() and is_sentinel(only_cover[0]).all()
            assert np.array_equal(only_start[0].view(np.uint64), got[0].view(np.uint64)) and np.array_equal(only_cover[1].view(np.uint64), got[1].view(np.uint64))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nl", [4, 7])
def test_cross_tie_with_the_expected_counts(ctx, nl, mode):
    """the device's start map pushed through the tree by letter is pfmscan_expect_staged's matrix; occ and windows are the occupancy's"""
    rng = np.random.default_rng(31 + nl + mode)
    m = 6
    codes, off, lens = rules.stream(rng, [0, 3, m - 1, m, m + 1, 31 + m, 32 + m, 700, 1100], nl, foreign=0.004, case=nl == 7)
    T = rules.table(rng, m, nl, 0.6, 1.7)
    if nl == 4:
        start, _, occ, win = run(ctx, codes, None, off, lens, T, None, mode)
    else:
        start, _, occ, win = run(ctx, None, codes, off, lens, None, T, mode)
    ctx.stage(codes)
    E, occ_e, win_e = ctx.expect_staged(T, nl, mode, off, lens, 0)
    assert rules.same_bits(occ, occ_e) and np.array_equal(win, win_e)
    for r, (o, n) in enumerate(zip(off, lens)):
        _, has = orules.terms(codes, o, n, T, nl)
        want = np.zeros((m, 8))
        if has.size:
            want[:, :nl] = erules.tree_rows(rules.by_letter(start[0, o:o + n], codes[o:o + n], has, m, nl)).reshape(m, nl)
        assert rules.same_bits(want, E[r, 0]), r


@pytest.mark.parametrize("mode", MODES)
def test_independent_of_batch_and_place_in_the_stream(ctx, mode):
    rng = np.random.default_rng(37 + mode)
    m = 12
    lengths = [int(x) for x in rng.integers(0, 900, size=30)] + [2 * tile_of(m) + 7]
    codes, codes2, off, lens = prules.streams(rng, lengths, foreign_seq=0.002, foreign_struct=0.002, case=True)
    Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(2)])
    Ss = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(2)])
    base = check(ctx, codes, codes2, off, lens, Rs, Ss, mode)
    recs = [(codes[o:o + n], codes2[o:o + n]) for o, n in zip(off, lens)]

    def packed(order, lead=0):
        ln = np.asarray([recs[i][0].size for i in order], dtype=np.int64)
        of = np.zeros(ln.size, dtype=np.int64)
        of[1:] = np.cumsum(ln[:-1] + 1)
        of += lead
        c, c2 = np.full(int((ln + 1).sum()) + lead, 7, dtype=np.uint8), np.full(int((ln + 1).sum()) + lead, 7, dtype=np.uint8)
        for o, i in zip(of, order):
            c[o:o + recs[i][0].size], c2[o:o + recs[i][0].size] = recs[i]
        return c, c2, of, ln

    def per_record(got, of, ln):
        return [(got[0][:, o:o + n], got[1][:, o:o + n]) for o, n in zip(of, ln)]

    want = per_record(base, off, lens)
    cut = 13
    parts = []
    for order, lead in ((range(cut), 0), (range(cut, len(recs)), 3)):
        c, c2, of, ln = packed(order, lead)
        got = run(ctx, c, c2, of, ln, Rs, Ss, mode)
        parts += per_record(got, of, ln)
        assert rules.same_bits(got[2], base[2][list(order)]) and np.array_equal(got[3], base[3][list(order)])
    for (s, c), (ws, wc) in zip(parts, want):
        assert rules.same_bits(s, ws) and rules.same_bits(c, wc)
    # either map alone equals both together
    only_start = run(ctx, codes, codes2, off, lens, Rs, Ss, mode, want_cover=False)
    only_cover = run(ctx, codes, codes2, off, lens, Rs, Ss, mode, want_start=False)
    assert only_start[1] is None and only_cover[0] is None
    assert rules.same_bits(only_start[0], base[0]) and rules.same_bits(only_cover[1], base[1])


def raw_events(ctx, R, S, mode, off, lens, thr, cap, fill=-7):
    """pfmscan_footprint_events_staged as it stands -> (rc, n_events, key, cover, start), the arrays pre-filled"""
    from rnascan_amd import _lib
    sq, st = ctx._footprint_tables(R, S)
    n_q, m = (sq if sq is not None else st).shape[:2]
    off, lens = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(lens, dtype=np.int64)
    key = np.full(max(cap, 1), fill, dtype=np.int64)
    cover, start = np.full(max(cap, 1), float(fill)), np.full(max(cap, 1), float(fill))
    k = ctypes.c_int64(-1)
    p = _lib._ptr
    rc = ctx._L.pfmscan_footprint_events_staged(ctx._h, p(sq), p(st), n_q, m, int(mode), p(off), p(lens), off.size, float(thr), cap, p(key), p(cover),
                                                p(start), ctypes.byref(k), None, None)
    return rc, int(k.value), key, cover, start


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pair", [False, True])
def test_events_are_the_filter_of_the_maps(ctx, pair, mode):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(43 + 2 * mode + pair)
    m = 12
    codes, codes2, off, lens = prules.streams(rng, [int(x) for x in rng.integers(0, 800, size=30)] + [0, 2 * tile_of(m) + 9],
                                              foreign_seq=0.002, foreign_struct=0.002)
    Rs = np.stack([rules.table(rng, m, 4, 0.3, 2.5) for _ in range(3)])
    Ss = np.stack([rules.table(rng, m, 7, 0.3, 2.5) for _ in range(3)]) if pair else None
    start, cover, occ, win = rules.footprint(codes, codes2, off, lens, Rs, Ss, mode)
    inside = np.zeros(codes.size, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    sparse = float(np.quantile(cover[:, inside], 0.98))
    attained = float(np.sort(cover[0, inside])[int(0.9 * inside.sum())])
    stage(ctx, codes, codes2)
    for thr in (attained, np.nextafter(attained, -np.inf), -np.inf, sparse):
        want = rules.events(start, cover, off, lens, thr)
        got = ctx.footprint_events_staged(Rs, Ss, mode, off, lens, thr)
        assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]) and (np.diff(got[0]) > 0).all()
        assert rules.same_bits(got[1], want[1]) and rules.same_bits(got[2], want[2])
        assert rules.same_bits(got[3], occ) and np.array_equal(got[4], win)
    at = int(np.flatnonzero((cover[0] == attained) & inside)[0])
    assert at not in set(rules.events(start, cover, off, lens, attained)[0].tolist())
    assert at in set(rules.events(start, cover, off, lens, np.nextafter(attained, -np.inf))[0].tolist())
    assert rules.events(start, cover, off, lens, -np.inf)[0].size == 3 * int(inside.sum())
    share = rules.events(start, cover, off, lens, sparse)[0].size / (3.0 * inside.sum())
    assert 0.001 <= share <= 0.05
    # a capacity one short: the verdict names the capacity that suffices and nothing was written
    want = rules.events(start, cover, off, lens, sparse)
    k = int(want[0].size)
    rc, n, key, cv, sw = raw_events(ctx, Rs, Ss, mode, off, lens, sparse, k - 1)
    assert rc == _lib.E_CAPACITY and n == k and (key == -7).all() and (cv == -7).all() and (sw == -7).all()
    rc, n, key, cv, sw = raw_events(ctx, Rs, Ss, mode, off, lens, sparse, k)
    assert rc == 0 and n == k and np.array_equal(key, want[0]) and rules.same_bits(cv, want[1]) and rules.same_bits(sw, want[2])
    with pytest.raises(_lib.CapacityError) as e:
        ctx.footprint_events_staged(Rs, Ss, mode, off, lens, sparse, capacity=k - 1)
    assert e.value.required == k
    rc, n, key, cv, sw = raw_events(ctx, Rs, Ss, mode, off, lens, np.nan, k)
    assert rc == _lib.E_BADARG and (key == -7).all()
    # the _dev form: unordered, the total in the counter, only the first `capacity` stored
    d_codes, d_codes2 = torch.from_numpy(codes).cuda(), torch.from_numpy(codes2).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    for cap in (k + 5, k // 2):
        d_key = torch.full((k + 5,), -7, dtype=torch.int64, device="cuda")
        d_cv = torch.full((k + 5,), -7.0, dtype=torch.float64, device="cuda")
        d_sw = torch.full((k + 5,), -7.0, dtype=torch.float64, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.footprint_events_dev(Rs, Ss, mode, d_codes.data_ptr(), d_codes2.data_ptr() if pair else None, codes.size, d_off.data_ptr(), d_len.data_ptr(),
                                 len(off), sparse, cap, d_key.data_ptr(), d_cv.data_ptr(), d_sw.data_ptr(), d_n.data_ptr())
        ctx.synchronize()
        assert int(d_n.cpu()[0]) == k
        key, cv, sw = d_key.cpu().numpy(), d_cv.cpu().numpy(), d_sw.cpu().numpy()
        stored = min(cap, k)
        assert (key[stored:] == -7).all() and (cv[stored:] == -7).all()
        order = np.argsort(key[:stored])
        where = np.searchsorted(want[0], key[:stored][order])
        assert np.array_equal(want[0][where], key[:stored][order]) and (np.diff(key[:stored][order]) > 0).all()
        assert rules.same_bits(cv[:stored][order], want[1][where]) and rules.same_bits(sw[:stored][order], want[2][where])


def test_error_paths_write_nothing(ctx):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(47)
    codes, codes2, off, lens = prules.streams(rng, [50, 60, 70])
    d_codes, d_codes2 = torch.from_numpy(codes).cuda(), torch.from_numpy(codes2).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    d_start = torch.full((2, codes.size), -7.0, dtype=torch.float64, device="cuda")
    d_cover = torch.full((2, codes.size), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L, h, p = ctx._L, ctx._h, _lib._ptr
    R, S = np.ascontiguousarray(np.stack([rules.table(rng, 8, 4)] * 2)), np.ascontiguousarray(np.stack([rules.table(rng, 8, 7)] * 2))
    wide = np.ascontiguousarray(np.stack([rules.table(rng, 65, 7)] * 2))
    ptr = lambda t, shift=0: p(t.data_ptr() + shift) if t is not None else None

    def dev(R=R, S=S, n_mo=2, m=8, mode=1, c=d_codes, c2=d_codes2, shift=0, shift2=0, n_pos=codes.size, o=d_off, ln=d_len, n_rec=3, st=d_start, cv=d_cover):
        return L.pfmscan_footprint_dev(h, p(R), p(S), n_mo, m, mode, ptr(c, shift), ptr(c2, shift2), n_pos, ptr(o), ptr(ln), n_rec, ptr(st), ptr(cv),
                                       None, None)
    assert dev(m=0) == _lib.E_BADSHAPE and dev(R=wide, S=wide, m=65) == _lib.E_BADSHAPE
    assert dev(shift=4) == _lib.E_BADSHAPE and dev(shift2=8) == _lib.E_BADSHAPE
    assert dev(mode=2) == _lib.E_BADARG and dev(R=None, S=None) == _lib.E_BADARG
    assert dev(c=None) == _lib.E_BADARG and dev(c2=None) == _lib.E_BADARG and dev(o=None) == _lib.E_BADARG
    assert dev(st=None, cv=None) == _lib.E_BADARG                           # both maps NULL
    assert dev(n_pos=codes.size - 2) == _lib.E_BADARG
    swapped = torch.from_numpy(off[[1, 0, 2]].copy()).cuda()               # a bad record table: refused before a kernel forms an address
    torch.cuda.synchronize()
    assert dev(o=swapped) == _lib.E_BADARG
    assert dev(n_mo=0) == 0 and dev(n_rec=0) == 0
    ctx.synchronize()
    assert (d_start.cpu().numpy() == -7).all() and (d_cover.cpu().numpy() == -7).all()
    # a stream that is not needed may be NULL and misaligned
    assert dev(S=None, c2=None) == 0 and dev(R=None, c=None, shift2=0) == 0 and dev() == 0
    ctx.synchronize()
    want = rules.footprint(codes, codes2, off, lens, R, S, rules.POSTERIOR, fill=-7.0)
    assert rules.same_bits(d_start.cpu().numpy(), want[0]) and rules.same_bits(d_cover.cpu().numpy(), want[1])
    ctx.stage(codes)
    with pytest.raises(ValueError):
        ctx.footprint_staged(R, S, 1, off, lens)                            # no codes2 staged
    ctx.stage_codes2(codes2)
    for bad in (dict(mode=2), dict(want_start=False, want_cover=False)):
        with pytest.raises(ValueError):
            ctx.footprint_staged(R, S, **dict(dict(mode=1, rec_off=off, rec_len=lens), **bad))
    with pytest.raises(ValueError):
        ctx.footprint_staged(wide, wide, 1, off, lens)
    with pytest.raises(ValueError):
        ctx.footprint_staged(R, S, 1, off[[1, 0, 2]], lens)


def test_engine_methods(ctx):
    from rnascan_amd import pack, scanner
    rng = np.random.default_rng(53)
    e = scanner.HipEngine(0)
    try:
        lens = (5, 300, 0, 77)
        stream = pack.pack([rng.integers(0, 4, size=n).astype(np.uint8) for n in lens])
        letters = pack.pack([rng.integers(0, 7, size=n).astype(np.uint8) for n in lens])   # a structure-letter FASTA on its own: codes, no codes2
        R, S = rules.table(rng, 6, 4), rules.table(rng, 6, 7)
        ref = rules.RulesEngine()
        for mode in MODES:
            assert same(e.footprint(letters, None, S, mode), ref.footprint(letters, None, S, mode))
            assert same(e.footprint(stream, R, None, mode), ref.footprint(stream, R, None, mode))
        stream.codes2 = letters.codes
        for mode in MODES:
            want = ref.footprint(stream, R, S, mode)
            assert same(e.footprint(stream, R, S, mode), want)
            thr = float(np.quantile(want[1], 0.9))
            got, wev = e.footprint_events(stream, R, S, mode, thr), ref.footprint_events(stream, R, S, mode, thr)
            assert np.array_equal(got[0], wev[0]) and rules.same_bits(got[1], wev[1]) and rules.same_bits(got[2], wev[2])
    finally:
        e.close()
