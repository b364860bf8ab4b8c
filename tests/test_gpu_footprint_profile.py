"""The posterior site map on averaged-structure profiles (k_fp_profile_tiles, csrc/pfmscan_footprint_profile.hip) on the GPU
against the rules (tests/footprint_profile_rules.py): every comparison is on the float64 bit patterns (NaN == NaN), the int64
keys and Windows -- there is no tolerance in the contract."""
import ctypes

import numpy as np
import pytest

import expect_rules as erules
import footprint_profile_rules as rules
import footprint_rules as frules
import occupancy_profile_rules as prules
import occupancy_rules as orules
import pair_rules

pytestmark = pytest.mark.gpu

MODES = (rules.RATIO, rules.POSTERIOR)
DTYPES = (np.float32, np.float64)
SENTINEL = np.array([0x7FF8DEAD0000BEEF], dtype=np.uint64).view(np.float64)[0]   # a NaN with a payload nothing computes


def tile_of(m):
    from rnascan_amd import _lib
    return _lib.FOOTPRINT_PROFILE_SLOTS - (m - 1)


def run(ctx, codes, profile, off, lens, st, sq, mode, **kw):
    ctx.stage(codes if sq is not None else None, profile)
    return ctx.footprint_profile_staged(st, sq, mode, off, lens, **kw)


def want_of(codes, profile, off, lens, st, sq, mode, **kw):
    return rules.footprint(profile, off, lens, st, codes if sq is not None else None, sq, mode, **kw)


def same(got, want):
    return (rules.same_bits(got[0], want[0]) and rules.same_bits(got[1], want[1]) and rules.same_bits(got[2], want[2]) and
            got[3].dtype == np.int64 and np.array_equal(got[3], want[3]))


def check(ctx, codes, profile, off, lens, st, sq, mode):
    got = run(ctx, codes, profile, off, lens, st, sq, mode)
    want = want_of(codes, profile, off, lens, st, sq, mode)
    for name, g, w in zip(("start", "cover", "occ"), got, want):
        assert rules.same_bits(g, w), "%s bits differ at %s" % (name, np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])
    assert got[3].dtype == np.int64 and np.array_equal(got[3], want[3])
    return got


def to_the_end(codes, profile):
    """without the last separator: the last record ends at the stream's end (its last 16-byte vector is cut short)"""
    return codes[:-1].copy(), profile[:-1].copy()


def ladder(rng, m):
    """every length 0 .. 3 m + 2; n_win and L around the kernel's tile; n_win 1, 32, 1024; short records in between, so that
    the records start at every residue of the row offset"""
    tile = tile_of(m)
    around = [n + m - 1 for n in (tile - 1, tile, tile + 1, 2 * tile + 1, 1, 32, 1024)] + [tile - 1, tile, tile + 1, 2 * tile + 1]
    lengths = list(range(0, 3 * m + 3))
    for x in around:
        lengths += [x, int(rng.integers(0, 2 * m + 2))]
    return lengths


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("m", [1, 2, 8, 12, 33, 64])
def test_length_ladder(ctx, m, joint, dtype):
    rng = np.random.default_rng(700 + 4 * m + 2 * joint + (dtype == np.float64))
    codes, profile, off, lens = prules.stream(rng, ladder(rng, m), dtype, foreign=0.002 if joint else 0.0)
    codes, profile = to_the_end(codes, profile)
    assert off[-1] + lens[-1] == codes.size and np.isnan(profile[off[3] + lens[3]]).all()
    n_win, tile = np.maximum(lens - m + 1, 0), tile_of(m)
    for n in (tile - 1, tile, tile + 1, 2 * tile + 1):
        assert (n_win == n).any() and (lens == n).any()
    for n in (1, 32, 1024):
        assert (n_win == n).any()
    for L in range(0, 3 * m + 3):
        assert (lens == L).any()
    assert len(set(int(o * 7 * profile.itemsize) % 16 for o in off)) == (4 if dtype == np.float32 else 2)
    st = prules.struct_table(rng, m, 0.6, 1.7)
    sq = orules.table(rng, m, 4, 0.6, 1.7) if joint else None
    for mode in MODES:
        start, cover, occ, win = check(ctx, codes, profile, off, lens, st, sq, mode)
        for o, n in zip(off, lens):                                # the record's last min(m - 1, L) starts, and the separator behind it
            assert (start[0, o + max(n - m + 1, 0):o + n + 1] == 0).all() and not np.signbit(start[0, o + max(n - m + 1, 0):o + n + 1]).any()
            assert o + n == codes.size or (cover[0, o + n] == 0 and not np.signbit(cover[0, o + n]))
        if mode == rules.POSTERIOR:
            for o, n, nw in zip(off, lens, n_win):
                if nw > 0:
                    assert cover[0, o:o + n].max() <= rules.cover_bound(int(nw), m)
    o2, w2 = ctx.occupancy_profile_staged(st, sq, off, lens)
    assert rules.same_bits(o2, occ) and np.array_equal(w2, win)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 8, 21])
def test_joint_foreign_codes(ctx, m, dtype):
    rng = np.random.default_rng(13 * m + (dtype == np.float64))
    L = 2 * m + 37
    codes, profile, off, lens = prules.stream(rng, [L] * (L + 1) + [3 * m + 150, tile_of(m) + 3 * m], dtype)
    for p in range(L):                                             # record p: one foreign code at position p (every offset of a window)
        codes[off[p] + p] = np.uint8(rng.integers(4, 8))
    codes[off[L]:off[L] + L] = 7                                   # a record of nothing else
    codes[off[-2] + 60] = codes[off[-2] + 60 + max(m - 1, 1)] = 5  # two within m
    t = tile_of(m)
    codes[off[-1] + t - 1] = codes[off[-1] + t + m - 1] = 6        # on either side of a tile's edge
    st, sq = prules.struct_table(rng, m), orules.table(rng, m, 4)
    for mode in MODES:
        start, cover, occ, win = check(ctx, codes, profile, off, lens, st, sq, mode)
        assert win[L] == 0 and occ[L, 0] == 0 and (start[0, off[L]:off[L] + L] == 0).all() and (cover[0, off[L]:off[L] + L] == 0).all()
        assert not np.signbit(cover[0, off[L]:off[L] + L]).any()
        assert win[0] == L - m and win[L - 1] == L - m
        # structure only: the codes are not read
        check(ctx, codes, profile, off, lens, st, None, mode)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("joint", [False, True])
def test_special_cells(ctx, joint, dtype):
    """a zero row, +inf * 0, NaN and negative cells, a record whose occupancy is NEGATIVE (its weights are t * (1 / occ), not
    zero: the decision is on occ == 0.0, never on the sign of 1 / occ), and weights that are -0.0"""
    rng = np.random.default_rng(59 + joint)
    m = 5                                                          # odd: m negative marginals make a negative term
    lengths = [40, 300, 33, 64, 70, 90, tile_of(m) + 20, 50]
    codes, profile, off, lens = prules.stream(rng, lengths, dtype, foreign=0.01 if joint else 0.0)
    profile[off[0] + 7] = 0.0                                      # a zero row: the m windows over it are +0.0
    profile[off[1]:off[1] + lens[1]] = 0.0                         # nothing but zero rows: occupancy 0, every weight +0.0
    profile[off[3]:off[3] + lens[3]] *= -1                         # every cell <= 0: every term <= 0, the occupancy negative
    profile[off[4] + 11, 2] = np.nan
    profile[off[5] + 5:off[5] + 9] *= -1                           # negative cells in a positive record: weights of both signs
    profile[off[6]:off[6] + lens[6]] *= -1                         # a negative record over a tile edge
    profile[off[6] + tile_of(m) - 2] = 0.0                         # with -0.0 weights on both sides of it (0 * negative)
    profile[off[7] + 20] = -0.0 * np.ones(7, dtype=dtype)          # -0.0 cells: a -0.0 marginal, -0.0 terms in a positive record
    st = np.stack([prules.struct_table(rng, m) for _ in range(3)])
    st[1, 2, 4] = np.inf                                           # inf * 0 where the row's cell 4 is 0: NaN
    st[2, 1, :] = 0.0                                              # a zero table row: every term +0.0 (or NaN), occupancy 0
    sq = np.stack([orules.table(rng, m, 4) for _ in range(3)]) if joint else None
    for mode in MODES:
        start, cover, occ, win = check(ctx, codes, profile, off, lens, st, sq, mode)
        assert occ[1, 0] == 0 and (start[0, off[1]:off[1] + lens[1]] == 0).all() and not np.signbit(cover[0, off[1]:off[1] + lens[1]]).any()
        assert occ[3, 0] < 0 and occ[6, 0] < 0
        inside3 = start[0, off[3]:off[3] + lens[3] - m + 1]
        if mode == rules.POSTERIOR:
            assert (inside3 >= 0).all() and 0.99 < inside3.sum() < 1.01   # t * (1 / occ), negative times negative: not zero
        else:
            assert (inside3 <= 0).all() and (inside3 < 0).any()
        assert np.isnan(cover[0, off[4]:off[4] + lens[4]]).any() and np.isnan(occ[4, 0])
        assert np.isnan(occ[:, 1]).any()                           # inf * 0
        assert (occ[:, 2] == 0).all() or np.isnan(occ[:, 2]).any()
        assert np.signbit(start[0][start[0] == 0]).any()           # a -0.0 weight is stored as it is
        assert (start[0, off[5]:off[5] + lens[5]] < 0).any() and (start[0, off[5]:off[5] + lens[5]] > 0).any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [1, 5, 12])
def test_one_hot_rows_equal_the_letter_form_on_the_device(ctx, m, mode):
    """rows that are one-hot in the structure letters: 1 * S + 0 * S ... = S exactly, so the maps are pfmscan_footprint_staged's
    on the letter codes (structure only) and on the two code streams (joint), bit for bit"""
    rng = np.random.default_rng(41 + m + mode)
    lengths = [int(x) for x in rng.integers(0, 500, size=30)] + [2 * tile_of(m) + 9]
    codes, letters, off, lens = pair_rules.streams(rng, lengths, foreign_seq=0.004, foreign_struct=0.0)
    S = prules.struct_table(rng, m)
    R8 = np.full((m, 8), np.nan)
    R8[:, :7] = S
    sq = orules.table(rng, m, 4)
    ctx.stage(codes)
    ctx.stage_codes2(letters)
    want_s = ctx.footprint_staged(None, R8, mode, off, lens)
    want_j = ctx.footprint_staged(sq, R8, mode, off, lens)
    for dtype in DTYPES:
        profile = prules.one_hot(letters, dtype)
        assert same(run(ctx, codes, profile, off, lens, S, None, mode), want_s)
        assert same(run(ctx, codes, profile, off, lens, S, sq, mode), want_j)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("joint", [False, True])
def test_weight_tie_with_the_expected_counts(ctx, joint, mode, dtype):
    """the device's start plane pushed through sum_s start[s] * r[s + k][c] with the tree of the expected counts is
    pfmscan_expect_profile_staged's exp_struct, bit for bit"""
    rng = np.random.default_rng(31 + 2 * joint + mode)
    m = 6
    codes, profile, off, lens = prules.stream(rng, [0, 3, m - 1, m, m + 1, 31 + m, 32 + m, 700, 1100], dtype, foreign=0.004 if joint else 0.0)
    st = prules.struct_table(rng, m, 0.6, 1.7)
    sq = orules.table(rng, m, 4, 0.6, 1.7) if joint else None
    start, _, occ, win = run(ctx, codes, profile, off, lens, st, sq, mode)
    ctx.stage(codes if joint else None, profile)
    Es, _, occ_e, win_e = ctx.expect_profile_staged(st, sq, mode, off, lens)
    assert rules.same_bits(occ, occ_e) and np.array_equal(win, win_e)
    for r, (o, n) in enumerate(zip(off, lens)):
        _, has = prules.terms(profile, o, n, st, codes if joint else None, sq)
        want = np.zeros((m, 8))
        if has.size:
            n_win = has.size
            x = profile[o:o + n].astype(np.float64)
            X = np.zeros((m * 7, n_win))
            with np.errstate(all="ignore"):
                for k in range(m):
                    for c in range(7):
                        X[k * 7 + c] = np.where(has, start[0, o:o + n_win] * x[k:k + n_win, c], 0.0)
            want[:, :7] = erules.tree_rows(X).reshape(m, 7)
        assert rules.same_bits(want, Es[r, 0]), r


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_motifs", [1, 3, 33])
def test_motifs_of_one_call_equal_one_call_each(ctx, n_motifs, dtype):
    rng = np.random.default_rng(23 + n_motifs)
    m = 9
    codes, profile, off, lens = prules.stream(rng, [int(x) for x in rng.integers(0, 260, size=12)] + [tile_of(m) + 30], dtype, foreign=0.004)
    st = np.stack([prules.struct_table(rng, m, 0.6, 1.7) for _ in range(n_motifs)])
    sq = np.stack([orules.table(rng, m, 4, 0.6, 1.7) for _ in range(n_motifs)])
    for tabs in (None, sq):
        got = check(ctx, codes, profile, off, lens, st, tabs, rules.POSTERIOR)
        for q in sorted(set((0, n_motifs // 2, n_motifs - 1))):
            one = run(ctx, codes, profile, off, lens, st[q], None if tabs is None else tabs[q], rules.POSTERIOR)
            assert same(one, (got[0][q:q + 1], got[1][q:q + 1], got[2][:, q:q + 1], got[3]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_independent_of_order_batch_place_plane_and_scratch(ctx, dtype, monkeypatch):
    rng = np.random.default_rng(37)
    m = 12
    lengths = [int(x) for x in rng.integers(0, 600, size=24)] + [2 * tile_of(m) + 7]
    codes, profile, off, lens = prules.stream(rng, lengths, dtype, foreign=0.003)
    st = np.stack([prules.struct_table(rng, m, 0.6, 1.7) for _ in range(2)])
    sq = np.stack([orules.table(rng, m, 4, 0.6, 1.7) for _ in range(2)])
    recs = [(codes[o:o + n], profile[o:o + n]) for o, n in zip(off, lens)]

    def packed(order, lead=0):
        ln = np.asarray([recs[i][0].size for i in order], dtype=np.int64)
        of = np.zeros(ln.size, dtype=np.int64)
        of[1:] = np.cumsum(ln[:-1] + 1)
        of += lead                                                 # `lead` rows that belong to no record come first
        c = np.full(int((ln + 1).sum()) + lead, 7, dtype=np.uint8)
        p = np.full((c.size, 7), np.nan, dtype=dtype)
        for o, i in zip(of, order):
            c[o:o + recs[i][0].size], p[o:o + recs[i][0].size] = recs[i]
        return c, p, of, ln

    def per_record(got, of, ln):
        return [(got[0][:, o:o + n], got[1][:, o:o + n]) for o, n in zip(of, ln)]

    for tabs in (None, sq):
        for mode in MODES:
            base = check(ctx, codes, profile, off, lens, st, tabs, mode)
            want = per_record(base, off, lens)
            order = [int(i) for i in rng.permutation(len(recs))]
            cut = 11
            for sel, lead in ((order, 0), (list(range(cut)), 0), (list(range(cut, len(recs))), 0), (list(range(len(recs))), 1),
                              (list(range(len(recs))), 2), (list(range(len(recs))), 3)):
                c, p, of, ln = packed(sel, lead)
                got = run(ctx, c, p, of, ln, st, tabs, mode)
                assert rules.same_bits(got[2], base[2][sel]) and np.array_equal(got[3], base[3][sel])
                for (s, cv), i in zip(per_record(got, of, ln), sel):
                    assert rules.same_bits(s, want[i][0]) and rules.same_bits(cv, want[i][1])
            # either plane alone equals both together
            only_start = run(ctx, codes, profile, off, lens, st, tabs, mode, want_cover=False)
            only_cover = run(ctx, codes, profile, off, lens, st, tabs, mode, want_start=False)
            assert only_start[1] is None and only_cover[0] is None
            assert rules.same_bits(only_start[0], base[0]) and rules.same_bits(only_cover[1], base[1])
            # the occupancy inside goes through bounded scratch: with a bound of a few cells no bit moves
            for cap in ("1", "50"):
                monkeypatch.setenv("PFMSCAN_OCC_SCRATCH_DOUBLES", cap)
                assert same(run(ctx, codes, profile, off, lens, st, tabs, mode), base)
            monkeypatch.delenv("PFMSCAN_OCC_SCRATCH_DOUBLES")


def raw_events(ctx, st, sq, mode, off, lens, thr, cap, fill=-7):
    """pfmscan_footprint_profile_events_staged as it stands -> (rc, n_events, key, cover, start), the arrays pre-filled"""
    from rnascan_amd import _lib
    st, sq = ctx._profile_tables(st, sq)
    n_q, m = st.shape[:2]
    off, lens = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(lens, dtype=np.int64)
    key = np.full(max(cap, 1), fill, dtype=np.int64)
    cover, start = np.full(max(cap, 1), float(fill)), np.full(max(cap, 1), float(fill))
    k = ctypes.c_int64(-1)
    p = _lib._ptr
    rc = ctx._L.pfmscan_footprint_profile_events_staged(ctx._h, p(st), p(sq), n_q, m, int(mode), p(off), p(lens), off.size, float(thr), cap, p(key),
                                                        p(cover), p(start), ctypes.byref(k), None, None)
    return rc, int(k.value), key, cover, start


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("joint", [False, True])
def test_events_are_the_filter_of_the_maps(ctx, joint, mode, dtype):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(43 + 2 * mode + joint)
    m = 12
    codes, profile, off, lens = prules.stream(rng, [int(x) for x in rng.integers(0, 500, size=24)] + [0, 2 * tile_of(m) + 9], dtype,
                                              foreign=0.002 if joint else 0.0)
    profile[off[2] + 9, 1] = np.nan                                # covers that are NaN: they pass no threshold, not even -inf
    st = np.stack([prules.struct_table(rng, m, 0.3, 2.5) for _ in range(3)])
    sq = np.stack([orules.table(rng, m, 4, 0.3, 2.5) for _ in range(3)]) if joint else None
    start, cover, occ, win = want_of(codes, profile, off, lens, st, sq, mode)
    inside = np.zeros(codes.size, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    finite = cover[:, inside][~np.isnan(cover[:, inside])]
    sparse = float(np.quantile(finite, 0.98))
    ctx.stage(codes if joint else None, profile)
    for thr in (0.5, -np.inf, np.inf, sparse):
        want = rules.events(start, cover, off, lens, thr)
        got = ctx.footprint_profile_events_staged(st, sq, mode, off, lens, thr)
        assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]) and (np.diff(got[0]) > 0).all()
        assert rules.same_bits(got[1], want[1]) and rules.same_bits(got[2], want[2])
        assert rules.same_bits(got[3], occ) and np.array_equal(got[4], win)
    assert rules.events(start, cover, off, lens, -np.inf)[0].size == int((~np.isnan(cover[:, inside])).sum()) < 3 * int(inside.sum())
    assert rules.events(start, cover, off, lens, np.inf)[0].size == 0
    # a capacity one short: the verdict names the capacity that suffices and nothing was written
    want = rules.events(start, cover, off, lens, sparse)
    k = int(want[0].size)
    assert k > 20
    rc, n, key, cv, sw = raw_events(ctx, st, sq, mode, off, lens, sparse, k - 1)
    assert rc == _lib.E_CAPACITY and n == k and (key == -7).all() and (cv == -7).all() and (sw == -7).all()
    rc, n, key, cv, sw = raw_events(ctx, st, sq, mode, off, lens, sparse, k)
    assert rc == 0 and n == k and np.array_equal(key, want[0]) and rules.same_bits(cv, want[1]) and rules.same_bits(sw, want[2])
    with pytest.raises(_lib.CapacityError) as e:
        ctx.footprint_profile_events_staged(st, sq, mode, off, lens, sparse, capacity=k - 1)
    assert e.value.required == k
    rc, n, key, cv, sw = raw_events(ctx, st, sq, mode, off, lens, np.nan, k)
    assert rc == _lib.E_BADARG and (key == -7).all()
    # the _dev form: unordered, the total in the counter, only the first `capacity` stored
    d_codes, d_prof = torch.from_numpy(codes).cuda(), torch.from_numpy(profile).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    for cap in (k + 5, k // 2):
        d_key = torch.full((k + 5,), -7, dtype=torch.int64, device="cuda")
        d_cv = torch.full((k + 5,), -7.0, dtype=torch.float64, device="cuda")
        d_sw = torch.full((k + 5,), -7.0, dtype=torch.float64, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.footprint_profile_events_dev(st, sq, mode, d_codes.data_ptr() if joint else None, d_prof.data_ptr(),
                                         _lib.PROFILE_F32 if dtype == np.float32 else _lib.PROFILE_F64, codes.size,
                                         d_off.data_ptr(), d_len.data_ptr(), len(off), sparse, cap, d_key.data_ptr(), d_cv.data_ptr(),
                                         d_sw.data_ptr(), d_n.data_ptr())
        ctx.synchronize()
        assert int(d_n.cpu()[0]) == k
        key, cv, sw = d_key.cpu().numpy(), d_cv.cpu().numpy(), d_sw.cpu().numpy()
        stored = min(cap, k)
        assert (key[stored:] == -7).all() and (cv[stored:] == -7).all()
        order = np.argsort(key[:stored])
        where = np.searchsorted(want[0], key[:stored][order])
        assert np.array_equal(want[0][where], key[:stored][order]) and (np.diff(key[:stored][order]) > 0).all()
        assert rules.same_bits(cv[:stored][order], want[1][where]) and rules.same_bits(sw[:stored][order], want[2][where])


def is_sentinel(x):
    return np.asarray(x).view(np.uint64) == SENTINEL.view(np.uint64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dev_form_as_an_integrator_calls_it(ctx, dtype):
    """separate device arrays pre-filled with a sentinel; positions in no record (separators, records the table skips) stay
    sentinel; one context serves the family's other calls back to back"""
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(29)
    m, n_mo = 8, 2
    codes, profile, off, lens = prules.stream(rng, [int(x) for x in rng.integers(0, 500, size=20)] + [tile_of(m) + 300], dtype, foreign=0.003)
    letters = rng.integers(0, 7, size=codes.size).astype(np.uint8)
    keep = np.array([i for i in range(len(off)) if i % 3 != 1])    # a table that skips records
    st = np.stack([prules.struct_table(rng, m) for _ in range(n_mo)])
    sq = np.stack([orules.table(rng, m, 4) for _ in range(n_mo)])
    code = _lib.PROFILE_F32 if dtype == np.float32 else _lib.PROFILE_F64
    d_codes, d_prof = torch.from_numpy(codes).cuda(), torch.from_numpy(profile).cuda()
    d_off, d_len = torch.from_numpy(off[keep].copy()).cuda(), torch.from_numpy(lens[keep].copy()).cuda()
    inside = np.zeros(codes.size, dtype=bool)
    for o, n in zip(off[keep], lens[keep]):
        inside[o:o + n] = True
    for tabs in (None, sq):
        for mode in MODES:
            want = want_of(codes, profile, off[keep], lens[keep], st, tabs, mode, fill=SENTINEL)
            planes = {}
            for name, ws, wc in (("both", True, True), ("start", True, False), ("cover", False, True)):
                d_start = torch.from_numpy(np.full((n_mo, codes.size), SENTINEL)).cuda()
                d_cover = torch.from_numpy(np.full((n_mo, codes.size), SENTINEL)).cuda()
                d_occ = torch.full((len(keep), n_mo), -7.0, dtype=torch.float64, device="cuda")
                d_win = torch.full((len(keep),), -7, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                ctx.footprint_profile_dev(st, tabs, mode, d_codes.data_ptr() if tabs is not None else None, d_prof.data_ptr(), code, codes.size,
                                          d_off.data_ptr(), d_len.data_ptr(), len(keep), d_start.data_ptr() if ws else None,
                                          d_cover.data_ptr() if wc else None, d_occ.data_ptr(), d_win.data_ptr())
                ctx.synchronize()
                planes[name] = (d_start.cpu().numpy(), d_cover.cpu().numpy())
                assert rules.same_bits(d_occ.cpu().numpy(), want[2]) and np.array_equal(d_win.cpu().numpy(), want[3])
            for g, w in zip(planes["both"], want):
                assert is_sentinel(g[:, ~inside]).all() and rules.same_bits(g[:, inside], w[:, inside])
            assert is_sentinel(planes["start"][1]).all() and is_sentinel(planes["cover"][0]).all()
            assert np.array_equal(planes["start"][0].view(np.uint64), planes["both"][0].view(np.uint64))
            assert np.array_equal(planes["cover"][1].view(np.uint64), planes["both"][1].view(np.uint64))
    # one context, the family back to back: every call's buffers are its own or re-made
    ctx.stage(codes, profile)
    ctx.stage_codes2(letters)
    a = ctx.footprint_profile_staged(st, sq, rules.POSTERIOR, off, lens)
    o1 = ctx.occupancy_profile_staged(st, sq, off, lens)
    e1 = ctx.expect_profile_staged(st, sq, rules.POSTERIOR, off, lens)
    f1 = ctx.footprint_staged(sq, None, rules.POSTERIOR, off, lens)
    b = ctx.footprint_profile_staged(st, sq, rules.POSTERIOR, off, lens)
    assert same(a, b) and same(a, want_of(codes, profile, off, lens, st, sq, rules.POSTERIOR))
    assert rules.same_bits(o1[0], a[2]) and rules.same_bits(e1[2], a[2])
    assert frules.same_bits(f1[0], frules.footprint(codes, None, off, lens, sq, None, frules.POSTERIOR)[0])


def test_bad_arguments_launch_nothing(ctx):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(47)
    codes, profile, off, lens = prules.stream(rng, [50, 60, 70], np.float32)
    d_codes, d_prof = torch.from_numpy(codes).cuda(), torch.from_numpy(profile).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    d_start = torch.full((2, codes.size), -7.0, dtype=torch.float64, device="cuda")
    d_cover = torch.full((2, codes.size), -7.0, dtype=torch.float64, device="cuda")
    d_occ = torch.full((3, 2), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L, h, p = ctx._L, ctx._h, _lib._ptr
    S = np.ascontiguousarray(np.stack([prules.struct_table(rng, 8)] * 2))
    R = np.ascontiguousarray(np.stack([orules.table(rng, 8, 4)] * 2))
    wide = np.ascontiguousarray(np.stack([prules.struct_table(rng, 65)] * 2))
    ptr = lambda t, shift=0: p(t.data_ptr() + shift) if t is not None else None

    def dev(st=S, sq=None, n_mo=2, m=8, mode=1, c=d_codes, prof=d_prof, dt=_lib.PROFILE_F32, shift=0, shift_prof=0, n_pos=codes.size, o=d_off,
            ln=d_len, n_rec=3, sta=d_start, cv=d_cover):
        return L.pfmscan_footprint_profile_dev(h, p(st), p(sq), n_mo, m, mode, ptr(c, shift), ptr(prof, shift_prof), dt, n_pos, ptr(o), ptr(ln), n_rec,
                                               ptr(sta), ptr(cv), ptr(d_occ), None)
    assert dev(m=0) == _lib.E_BADSHAPE and dev(st=wide, m=65) == _lib.E_BADSHAPE
    assert dev(shift_prof=4) == _lib.E_BADSHAPE and dev(sq=R, shift=4) == _lib.E_BADSHAPE
    assert dev(dt=7) == _lib.E_BADARG and dev(mode=2) == _lib.E_BADARG
    assert dev(st=None) == _lib.E_BADARG and dev(st=None, sq=R) == _lib.E_BADARG        # struct_tables is required
    assert dev(sq=R, c=None) == _lib.E_BADARG                                          # joint mode needs the codes
    assert dev(prof=None) == _lib.E_BADARG and dev(o=None) == _lib.E_BADARG and dev(ln=None) == _lib.E_BADARG
    assert dev(sta=None, cv=None) == _lib.E_BADARG                                     # both planes NULL
    assert dev(n_pos=codes.size - 2) == _lib.E_BADARG and dev(n_mo=-1) == _lib.E_BADARG and dev(n_rec=-1) == _lib.E_BADARG
    swapped = torch.from_numpy(off[[1, 0, 2]].copy()).cuda()      # a bad record table: refused before a kernel forms an address
    torch.cuda.synchronize()
    assert dev(o=swapped) == _lib.E_BADARG
    assert dev(n_mo=0) == 0 and dev(n_rec=0) == 0
    ctx.synchronize()
    assert (d_start.cpu().numpy() == -7).all() and (d_cover.cpu().numpy() == -7).all() and (d_occ.cpu().numpy() == -7).all()
    # structure only: the codes may be NULL and misaligned
    assert dev(c=None) == 0 and dev(shift=4) == 0
    ctx.synchronize()
    want = rules.footprint(profile, off, lens, S, None, None, rules.POSTERIOR, fill=-7.0)
    assert rules.same_bits(d_start.cpu().numpy(), want[0]) and rules.same_bits(d_cover.cpu().numpy(), want[1])
    assert rules.same_bits(d_occ.cpu().numpy(), want[2])
    # the _staged form: what is staged, then the same checks
    ctx.stage(codes)
    with pytest.raises(ValueError):
        ctx.footprint_profile_staged(S, None, 1, off, lens)        # no profile staged
    ctx.stage(None, profile)
    with pytest.raises(ValueError):
        ctx.footprint_profile_staged(S, R, 1, off, lens)           # no codes staged
    ctx.stage(codes, profile)
    for bad in (dict(mode=2), dict(want_start=False, want_cover=False)):
        with pytest.raises(ValueError):
            ctx.footprint_profile_staged(S, R, **dict(dict(mode=1, rec_off=off, rec_len=lens), **bad))
    with pytest.raises(ValueError):
        ctx.footprint_profile_staged(wide, None, 1, off, lens)
    with pytest.raises(ValueError):
        ctx.footprint_profile_staged(S, R, 1, off[[1, 0, 2]], lens)
    k = ctypes.c_int64(-1)
    rc = L.pfmscan_footprint_profile_events_staged(h, None, None, 2, 8, 1, p(off), p(lens), 3, 0.5, 0, None, None, None, ctypes.byref(k), None, None)
    assert rc == _lib.E_BADARG and k.value == -1


def test_engine_methods(ctx):
    from rnascan_amd import pack, scanner
    rng = np.random.default_rng(53)
    e = scanner.HipEngine(0)
    try:
        lens = (5, 300, 0, 77)
        stream = pack.pack([rng.integers(0, 4, size=n).astype(np.uint8) for n in lens], [prules.rows(rng, n) for n in lens])
        st, sq = prules.struct_table(rng, 6), orules.table(rng, 6)
        ref = rules.RulesEngine()
        for mode in MODES:
            for tabs in (None, sq):
                want = ref.footprint_profile(stream, st, tabs, mode)
                assert same(e.footprint_profile(stream, st, tabs, mode), want)
                thr = float(np.quantile(want[1], 0.9))
                got, wev = e.footprint_profile_events(stream, st, tabs, mode, thr), ref.footprint_profile_events(stream, st, tabs, mode, thr)
                assert np.array_equal(got[0], wev[0]) and rules.same_bits(got[1], wev[1]) and rules.same_bits(got[2], wev[2])
    finally:
        e.close()
