"""The multi-site model on averaged-structure profiles (k_ms_profile_terms in csrc/pfmscan_multisite.hip, then the model's own
kernels) on the GPU against the rules (tests/multisite_profile_rules.py): every comparison is on the float64 bit patterns
(NaN == NaN), the int64 keys and Windows -- there is no tolerance in the contract."""
import ctypes

import numpy as np
import pytest

import multisite_profile_rules as rules
import occupancy_profile_rules as prules
import occupancy_rules as orules
import pair_rules

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
SENTINEL = np.array([0x7FF8DEAD0000BEEF], dtype=np.uint64).view(np.float64)[0]   # a NaN with a payload nothing computes
CAP_KNOB = "PFMSCAN_MULTISITE_SCRATCH_DOUBLES"
NAMES = ("start", "cover", "z", "nsites")


def tile_of(m):
    from rnascan_amd import _lib
    return _lib.MULTISITE_SLOTS - (m - 1)


def dtype_code(dtype):
    from rnascan_amd import _lib
    return _lib.PROFILE_F32 if dtype == np.float32 else _lib.PROFILE_F64


def run(ctx, codes, profile, off, lens, st, sq, lam, **kw):
    ctx.stage(codes if sq is not None else None, profile)
    return ctx.multisite_profile_staged(st, sq, off, lens, lam, **kw)


def want_of(codes, profile, off, lens, st, sq, lam, **kw):
    return rules.multisite(profile, off, lens, st, codes if sq is not None else None, sq, np.asarray(lam, dtype=np.float64), **kw)


def same(got, want):
    return (all(rules.same_bits(g, w) for g, w in zip(got[:4], want[:4])) and got[4].dtype == np.int64 and np.array_equal(got[4], want[4]))


def check(ctx, codes, profile, off, lens, st, sq, lam):
    got = run(ctx, codes, profile, off, lens, st, sq, lam)
    want = want_of(codes, profile, off, lens, st, sq, lam)
    for name, g, w in zip(NAMES, got, want):
        assert rules.same_bits(g, w), "%s bits differ at %s" % (name, np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])
    assert got[4].dtype == np.int64 and np.array_equal(got[4], want[4])
    return got


def lams(rng, n, hi=0.3):
    lam = rng.uniform(0.0, hi, size=n)
    lam[::7] = 0.0                                                 # +0.0: Z = 1.0 and no site
    return lam


def ladder(m):
    """the lengths of the ladder, descending then ascending: one stream, the record starts on every residue of the 16-byte
    alignment of float32 rows, the longest record last"""
    tile = tile_of(m)
    steps = sorted(set(max(x, 0) for x in (0, 1, m - 1, m, m + 1, 27, 28, 29, 57, tile - 1, tile, tile + 1, 2 * tile + 3)))
    lengths = steps[::-1] + steps
    if (sum(lengths) + len(lengths) - 1) % 2 == 0:                  # positions of the stream without its last separator: odd, so
        lengths = [0] + lengths                                    # that the last 16-byte vector of either dtype is cut short
    return lengths, steps


def to_the_end(codes, profile):
    """without the last separator: the last record ends at the stream's end (its last 16-byte vector is cut short)"""
    return codes[:-1].copy(), profile[:-1].copy()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("m", [1, 2, 8, 12, 33, 64])
def test_length_ladder(ctx, m, joint, dtype):
    rng = np.random.default_rng(1100 + 4 * m + 2 * joint + (dtype == np.float64))
    lengths, steps = ladder(m)
    codes, profile, off, lens = prules.stream(rng, lengths, dtype, foreign=0.002 if joint else 0.0)
    codes, profile = to_the_end(codes, profile)
    tile = tile_of(m)
    assert off[-1] + lens[-1] == codes.size and lens[-1] == 2 * tile + 3 and (codes.size * 7 * profile.itemsize) % 16 != 0
    assert np.isnan(profile[off[0] + lens[0]]).all()               # the separators hold NaN
    for L in (0, 1, m - 1, m, m + 1, 27, 28, 29, 57, tile - 1, tile, tile + 1, 2 * tile + 3):
        assert (lens == L).any()
    assert len(set(int(o * 7 * profile.itemsize) % 16 for o in off)) == (4 if dtype == np.float32 else 2)
    st = prules.struct_table(rng, m, 0.6, 1.7)
    sq = orules.table(rng, m, 4, 0.6, 1.7) if joint else None
    start, cover, z, ns, win = check(ctx, codes, profile, off, lens, st, sq, lams(rng, len(off)))
    assert not np.signbit(start).any() and not np.signbit(cover).any() and np.isfinite(z).all() and (z >= 1.0).all()
    for o, n, zz in zip(off, lens, z[:, 0]):                       # the record's last min(m - 1, L) starts, and the separator behind it
        assert (start[0, o + max(n - m + 1, 0):o + n] == 0).all()
        assert o + n == codes.size or (start[0, o + n] == 0 and cover[0, o + n] == 0)
        if n < m:
            assert zz == 1.0
        if n:
            assert cover[0, o:o + n].max() <= rules.cover_bound(int(n), m)
    o2, w2 = ctx.occupancy_profile_staged(st, sq, off, lens)       # Windows is the occupancy's count
    assert np.array_equal(w2, win)


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_pairs_than_a_wave_retire_at_different_steps(ctx, dtype):
    rng = np.random.default_rng(1201)
    m = 8
    lengths = [int(x) for x in rng.integers(0, 201, size=150)]
    lengths[40:40] = [3000, 0, 0]
    lengths[::31] = [0] * len(lengths[::31])
    codes, profile, off, lens = prules.stream(rng, lengths, dtype, foreign=0.002)
    assert len(off) > 64 and len(off) % 64 != 0
    st = np.stack([prules.struct_table(rng, m, 0.6, 1.7) for _ in range(3)])
    sq = np.stack([orules.table(rng, m, 4, 0.6, 1.7) for _ in range(3)])
    lam = lams(rng, len(off), 0.05)
    check(ctx, codes, profile, off, lens, st, None, lam)
    check(ctx, codes, profile, off, lens, st, sq, lam)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 8, 21])
def test_joint_foreign_codes(ctx, m, dtype):
    rng = np.random.default_rng(19 * m + (dtype == np.float64))
    L = 2 * m + 37
    t = tile_of(m)
    codes, profile, off, lens = prules.stream(rng, [L] * (L + 1) + [3 * m + 150, t + 3 * m, 2 * t + m], dtype)
    for p in range(L):                                             # record p: one foreign code at position p (every offset of a window)
        codes[off[p] + p] = np.uint8(rng.integers(4, 8))
    codes[off[L]:off[L] + L] = 7                                   # a record of nothing else
    codes[off[-3] + 60] = codes[off[-3] + 60 + max(m - 1, 1)] = 5  # two within m
    codes[off[-2] + t - 1] = codes[off[-2] + t + m - 1] = 6        # on either side of a tile's edge: the windows across it have no term
    codes[off[-1]] = 4                                             # in the first window of the first tile,
    codes[off[-1] + t + m - 1] = 5                                 # in the last window that begins in it (and the first of the next),
    codes[off[-1] + 2 * t - 1] = 6                                 # and in the last window of the second
    st, sq = prules.struct_table(rng, m), orules.table(rng, m, 4)
    lam = rng.uniform(0.01, 0.3, size=len(off))
    start, cover, z, ns, win = check(ctx, codes, profile, off, lens, st, sq, lam)
    assert win[L] == 0 and z[L, 0] == 1.0 and ns[L, 0] == 0 and (cover[0, off[L]:off[L] + L] == 0).all()
    assert win[0] == L - m and win[L - 1] == L - m
    assert start[0, off[-1]] == 0 and start[0, off[-1] + t] == 0
    check(ctx, codes, profile, off, lens, st, None, lam)           # structure only: the codes are not read


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("joint", [False, True])
def test_special_cells(ctx, joint, dtype):
    """negative, -0.0, infinite and NaN cells on either side of a tile edge, a zero row, 0 * inf from the table, and records
    whose Z is negative, zero-crossing or NaN: z, start and cover are the rule's bits, whatever they are"""
    rng = np.random.default_rng(1259 + joint)
    m = 5                                                          # odd: m negative marginals make a negative term
    t = tile_of(m)
    lengths = [40, 300, 33, 64, 70, 90, t + 20, 50, t + 40, t + 40, t + 40]
    codes, profile, off, lens = prules.stream(rng, lengths, dtype, foreign=0.01 if joint else 0.0)
    profile[off[0] + 7] = 0.0                                      # a zero row: the m windows over it are +0.0
    profile[off[1]:off[1] + lens[1]] = 0.0                         # nothing but zero rows: Z = 1.0
    profile[off[3]:off[3] + lens[3]] *= -1                         # every cell <= 0: every term <= 0
    profile[off[4] + 11, 2] = np.nan
    profile[off[5] + 5:off[5] + 9] *= -1                           # negative cells in a positive record
    profile[off[6]:off[6] + lens[6]] *= -1                         # a negative record over a tile edge
    profile[off[6] + t - 2] = 0.0
    profile[off[7] + 20] = -0.0 * np.ones(7, dtype=dtype)          # -0.0 cells
    for r, val in ((8, -3.0), (9, np.inf), (10, np.nan)):          # one cell before a tile's edge and one behind it
        profile[off[r] + t - 1, 1] = val
        profile[off[r] + t, 3] = val
    profile[off[8] + t + 7] = -0.0 * np.ones(7, dtype=dtype)
    st = np.stack([prules.struct_table(rng, m) for _ in range(3)])
    st[1, 2, 4] = np.inf                                           # inf * 0 where the row's cell 4 is 0: NaN
    st[2, 1, :] = 0.0                                              # a zero table row: every term +0.0 (or NaN)
    sq = np.stack([orules.table(rng, m, 4) for _ in range(3)]) if joint else None
    lam = rng.uniform(0.05, 0.5, size=len(off))
    lam[3] = 2.0
    start, cover, z, ns, win = check(ctx, codes, profile, off, lens, st, sq, lam)
    assert z[1, 0] == 1.0 and (start[0, off[1]:off[1] + lens[1]] == 0).all()
    assert (start[0, off[3]:off[3] + lens[3]] < 0).any() or z[3, 0] < 1.0          # negative activities
    assert np.isnan(z[4, 0]) and np.isnan(cover[0, off[4]:off[4] + lens[4]]).any()
    assert np.isnan(z[:, 1]).any()                                 # inf * 0
    assert np.isnan(z[10, 0]) and not np.isfinite(z[9, 0])
    assert np.isfinite(z[8, 0]) and (start[0, off[8]:off[8] + lens[8]] < 0).any()
    assert (z[:, 2] == 1.0).all() or np.isnan(z[:, 2]).any()
    # a Z that a negative cell drives to zero or below is returned as it is
    # (lam small: Z is 1 + the sum of the activities to first order, and the m windows over the cell outweigh the rest)
    profile[off[8] + t - 1, 1], profile[off[8] + t, 3] = -1e6, 0.25
    codes[off[8] + t - 1 - m:off[8] + t + m] = 0                   # letters: the windows over the cell have their terms
    start, cover, z, ns, win = check(ctx, codes, profile, off, lens, st[:1], None if sq is None else sq[:1], np.full(len(off), 1e-4))
    assert z[8, 0] < 0.0


@pytest.mark.parametrize("m", [1, 5, 12])
def test_one_hot_rows_equal_the_letter_form_on_the_device(ctx, m):
    """rows that are one-hot in the structure letters: 1 * S + 0 * S ... = S exactly, so the model is pfmscan_multisite_staged's
    on the letter codes (structure only) and on the two code streams (joint), bit for bit"""
    rng = np.random.default_rng(1241 + m)
    lengths = [int(x) for x in rng.integers(0, 500, size=30)] + [2 * tile_of(m) + 9]
    codes, letters, off, lens = pair_rules.streams(rng, lengths, foreign_seq=0.004, foreign_struct=0.0)
    S = prules.struct_table(rng, m)
    R8 = np.full((m, 8), np.nan)
    R8[:, :7] = S
    sq = orules.table(rng, m, 4)
    lam = lams(rng, len(off), 0.05)
    ctx.stage(codes)
    ctx.stage_codes2(letters)
    want_s = ctx.multisite_staged(None, R8, off, lens, lam)
    want_j = ctx.multisite_staged(sq, R8, off, lens, lam)
    for dtype in DTYPES:
        profile = prules.one_hot(letters, dtype)
        assert same(run(ctx, codes, profile, off, lens, S, None, lam), want_s)
        assert same(run(ctx, codes, profile, off, lens, S, sq, lam), want_j)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("joint", [False, True])
def test_term_tie_with_the_occupancy(ctx, joint, dtype):
    """plane A is not returned; with lam = 1.0 and a record of exactly one window, F[m] = 1.0 + t * 1.0: z - 1.0 is the term,
    which is the occupancy of that record (a tree of one leaf) -- where 1.0 + t is exact"""
    rng = np.random.default_rng(1277 + joint)
    m = 7
    codes, profile, off, lens = prules.stream(rng, [m] * 40, dtype)
    grid = np.arange(8) / 8.0                                      # rows and tables on a grid of 1/8 and powers of two: every product
    for o in off:                                                  # and sum of the chain is exact, and so is 1.0 + t
        profile[o:o + m] = rng.choice(grid, size=(m, 7)).astype(dtype)
    st = rng.choice([0.5, 1.0, 2.0], size=(m, 7))
    sq = None
    if joint:
        sq = np.full((m, 8), np.nan)
        sq[:, :4] = rng.choice([0.5, 1.0, 2.0], size=(m, 4))
        codes[off[5] + 3] = 6                                      # a window without a term: z = 1.0 + 0.0
    start, cover, z, ns, win = check(ctx, codes, profile, off, lens, st, sq, np.ones(len(off)))
    occ, w2 = ctx.occupancy_profile_staged(st, sq, off, lens)
    assert np.array_equal(win, w2) and (occ[:, 0] > 0).sum() > 20
    fits = (1.0 + occ[:, 0]) - 1.0 == occ[:, 0]
    assert fits.sum() > 20 and rules.same_bits((z[:, 0] - 1.0)[fits], occ[fits, 0])
    assert rules.same_bits(z[:, 0], 1.0 + occ[:, 0])               # every record: one rounded addition to 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_motifs", [1, 3, 33])
def test_motifs_of_one_call_equal_one_call_each(ctx, n_motifs, dtype):
    rng = np.random.default_rng(1223 + n_motifs)
    m = 9
    codes, profile, off, lens = prules.stream(rng, [int(x) for x in rng.integers(0, 260, size=12)] + [tile_of(m) + 30], dtype, foreign=0.004)
    st = np.stack([prules.struct_table(rng, m, 0.6, 1.7) for _ in range(n_motifs)])
    sq = np.stack([orules.table(rng, m, 4, 0.6, 1.7) for _ in range(n_motifs)])
    lam = lams(rng, len(off), 0.05)
    for tabs in (None, sq):
        got = check(ctx, codes, profile, off, lens, st, tabs, lam)
        for q in sorted(set((0, n_motifs // 2, n_motifs - 1))):
            one = run(ctx, codes, profile, off, lens, st[q], None if tabs is None else tabs[q], lam)
            assert same(one, (got[0][q:q + 1], got[1][q:q + 1], got[2][:, q:q + 1], got[3][:, q:q + 1], got[4]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_passes_over_records_and_motifs_do_not_change_the_bits(ctx, dtype, monkeypatch):
    rng = np.random.default_rng(1247)
    m = 12
    lengths = [int(x) for x in rng.integers(0, 700, size=30)] + [0, 1500]
    codes, profile, off, lens = prules.stream(rng, lengths, dtype, foreign=0.003)
    st = np.stack([prules.struct_table(rng, m, 0.6, 1.7) for _ in range(3)])
    sq = np.stack([orules.table(rng, m, 4, 0.6, 1.7) for _ in range(3)])
    lam = lams(rng, len(off), 0.05)
    monkeypatch.delenv(CAP_KNOB, raising=False)
    for tabs in (None, sq):
        one = check(ctx, codes, profile, off, lens, st, tabs, lam)
        assert one[4].sum() > 0
        want_ev = ctx.multisite_profile_events_staged(st, tabs, off, lens, lam, 0.01)
        n_pos = codes.size
        # 2: every record and motif a pass of its own; n_pos: several passes over records, one motif each; 4 n_pos: all
        # records, two motifs then one.  windows is counted in the pass of motif 0 only: the same counts
        for cap in (2, n_pos, 4 * n_pos + 8):
            monkeypatch.setenv(CAP_KNOB, str(cap))
            assert same(run(ctx, codes, profile, off, lens, st, tabs, lam), one), cap
            ev = ctx.multisite_profile_events_staged(st, tabs, off, lens, lam, 0.01)
            assert all(np.array_equal(np.asarray(g).view(np.uint64), np.asarray(w).view(np.uint64)) for g, w in zip(ev, want_ev)), cap
            monkeypatch.delenv(CAP_KNOB)


@pytest.mark.parametrize("dtype", DTYPES)
def test_independent_of_batch_place_and_planes(ctx, dtype):
    rng = np.random.default_rng(1237)
    m = 12
    lengths = [int(x) for x in rng.integers(0, 600, size=24)] + [2 * tile_of(m) + 7]
    codes, profile, off, lens = prules.stream(rng, lengths, dtype, foreign=0.003)
    st = np.stack([prules.struct_table(rng, m, 0.6, 1.7) for _ in range(2)])
    sq = np.stack([orules.table(rng, m, 4, 0.6, 1.7) for _ in range(2)])
    lam = lams(rng, len(off), 0.05)
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
        base = check(ctx, codes, profile, off, lens, st, tabs, lam)
        want = per_record(base, off, lens)
        order = [int(i) for i in rng.permutation(len(recs))]
        cut = 11
        for sel, lead in ((order, 0), (list(range(cut)), 0), (list(range(cut, len(recs))), 0), (list(range(len(recs))), 1),
                          (list(range(len(recs))), 2), (list(range(len(recs))), 3), ([len(recs) - 1], 1)):
            c, p, of, ln = packed(sel, lead)
            got = run(ctx, c, p, of, ln, st, tabs, lam[sel])
            assert rules.same_bits(got[2], base[2][sel]) and rules.same_bits(got[3], base[3][sel]) and np.array_equal(got[4], base[4][sel])
            for (s, cv), i in zip(per_record(got, of, ln), sel):
                assert rules.same_bits(s, want[i][0]) and rules.same_bits(cv, want[i][1])
        # either plane alone equals both together
        only_start = run(ctx, codes, profile, off, lens, st, tabs, lam, want_cover=False)
        only_cover = run(ctx, codes, profile, off, lens, st, tabs, lam, want_start=False)
        assert only_start[1] is None and only_cover[0] is None
        assert rules.same_bits(only_start[0], base[0]) and rules.same_bits(only_cover[1], base[1])
        assert rules.same_bits(only_start[2], base[2]) and rules.same_bits(only_cover[3], base[3])


def raw_events(ctx, st, sq, off, lens, lam, thr, cap, fill=-7):
    """pfmscan_multisite_profile_events_staged as it stands -> (rc, n_events, key, cover, start), the arrays pre-filled"""
    from rnascan_amd import _lib
    st, sq = ctx._profile_tables(st, sq)
    n_q, m = st.shape[:2]
    off, lens = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(lens, dtype=np.int64)
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    key = np.full(max(cap, 1), fill, dtype=np.int64)
    cover, start = np.full(max(cap, 1), float(fill)), np.full(max(cap, 1), float(fill))
    k = ctypes.c_int64(-1)
    p = _lib._ptr
    rc = ctx._L.pfmscan_multisite_profile_events_staged(ctx._h, p(st), p(sq), n_q, m, p(off), p(lens), off.size, p(lam), float(thr), cap, p(key),
                                                        p(cover), p(start), ctypes.byref(k), None, None, None)
    return rc, int(k.value), key, cover, start


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("joint", [False, True])
def test_events_are_the_filter_of_the_maps(ctx, joint, dtype):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(1249 + joint)
    m = 12
    codes, profile, off, lens = prules.stream(rng, [int(x) for x in rng.integers(0, 500, size=24)] + [0, 2 * tile_of(m) + 9], dtype,
                                              foreign=0.002 if joint else 0.0)
    profile[off[2] + 9, 1] = np.nan                                # covers that are NaN: they pass no threshold, not even -inf
    st = np.stack([prules.struct_table(rng, m, 0.3, 2.5) for _ in range(3)])
    sq = np.stack([orules.table(rng, m, 4, 0.3, 2.5) for _ in range(3)]) if joint else None
    lam = rng.uniform(0.001, 0.02, size=len(off))
    start, cover, z, ns, win = want_of(codes, profile, off, lens, st, sq, lam)
    inside = np.zeros(codes.size, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    finite = cover[:, inside][~np.isnan(cover[:, inside])]
    assert finite.size < cover[:, inside].size
    sparse = float(np.quantile(finite, 0.98))
    attained = float(np.sort(cover[0, inside & ~np.isnan(cover[0])])[int(0.9 * (inside & ~np.isnan(cover[0])).sum())])
    ctx.stage(codes if joint else None, profile)
    for thr in (attained, np.nextafter(attained, -np.inf), -np.inf, np.inf, sparse):
        want = rules.events(start, cover, off, lens, thr)
        got = ctx.multisite_profile_events_staged(st, sq, off, lens, lam, thr)
        assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]) and (np.diff(got[0]) > 0).all()
        assert rules.same_bits(got[1], want[1]) and rules.same_bits(got[2], want[2])
        assert rules.same_bits(got[3], z) and rules.same_bits(got[4], ns) and np.array_equal(got[5], win)
    at = int(np.flatnonzero((cover[0] == attained) & inside)[0])   # strict: a cover equal to thr is no event
    assert at not in set(rules.events(start, cover, off, lens, attained)[0].tolist())
    assert at in set(rules.events(start, cover, off, lens, np.nextafter(attained, -np.inf))[0].tolist())
    assert rules.events(start, cover, off, lens, -np.inf)[0].size == finite.size       # NaN never passes
    # a capacity one short: the verdict names the capacity that suffices and nothing was written
    want = rules.events(start, cover, off, lens, sparse)
    k = int(want[0].size)
    assert k > 20
    rc, n, key, cv, sw = raw_events(ctx, st, sq, off, lens, lam, sparse, k - 1)
    assert rc == _lib.E_CAPACITY and n == k and (key == -7).all() and (cv == -7).all() and (sw == -7).all()
    rc, n, key, cv, sw = raw_events(ctx, st, sq, off, lens, lam, sparse, k)
    assert rc == 0 and n == k and np.array_equal(key, want[0]) and rules.same_bits(cv, want[1]) and rules.same_bits(sw, want[2])
    with pytest.raises(_lib.CapacityError) as e:
        ctx.multisite_profile_events_staged(st, sq, off, lens, lam, sparse, capacity=k - 1)
    assert e.value.required == k
    rc, n, key, cv, sw = raw_events(ctx, st, sq, off, lens, lam, np.nan, k)
    assert rc == _lib.E_BADARG and (key == -7).all()
    # the _dev form: unordered, the total in the counter, only the first `capacity` stored
    d_codes, d_prof = torch.from_numpy(codes).cuda(), torch.from_numpy(profile).cuda()
    d_off, d_len, d_lam = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(lam).cuda()
    for cap in (k + 5, k // 2):
        d_key = torch.full((k + 5,), -7, dtype=torch.int64, device="cuda")
        d_cv = torch.full((k + 5,), -7.0, dtype=torch.float64, device="cuda")
        d_sw = torch.full((k + 5,), -7.0, dtype=torch.float64, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.multisite_profile_events_dev(st, sq, d_codes.data_ptr() if joint else None, d_prof.data_ptr(), dtype_code(dtype), codes.size,
                                         d_off.data_ptr(), d_len.data_ptr(), len(off), d_lam.data_ptr(), sparse, cap, d_key.data_ptr(),
                                         d_cv.data_ptr(), d_sw.data_ptr(), d_n.data_ptr())
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
    sentinel; every optional output NULL in turn; one context serves the family's other calls back to back"""
    import torch
    rng = np.random.default_rng(1229)
    m, n_mo = 8, 2
    codes, profile, off, lens = prules.stream(rng, [int(x) for x in rng.integers(0, 500, size=20)] + [tile_of(m) + 300], dtype, foreign=0.003)
    keep = np.array([i for i in range(len(off)) if i % 3 != 1])    # a table that skips records
    st = np.stack([prules.struct_table(rng, m) for _ in range(n_mo)])
    sq = np.stack([orules.table(rng, m, 4) for _ in range(n_mo)])
    lam = lams(rng, len(keep), 0.1)
    d_codes, d_prof = torch.from_numpy(codes).cuda(), torch.from_numpy(profile).cuda()
    d_off, d_len = torch.from_numpy(off[keep].copy()).cuda(), torch.from_numpy(lens[keep].copy()).cuda()
    d_lam = torch.from_numpy(lam).cuda()
    inside = np.zeros(codes.size, dtype=bool)
    for o, n in zip(off[keep], lens[keep]):
        inside[o:o + n] = True
    for tabs in (None, sq):
        want = want_of(codes, profile, off[keep], lens[keep], st, tabs, lam, fill=SENTINEL)
        planes = {}
        # (start, cover, z, nsites, windows) asked for
        for name, ask in (("all", (1, 1, 1, 1, 1)), ("start", (1, 0, 1, 1, 1)), ("cover", (0, 1, 1, 1, 1)), ("no z", (1, 1, 0, 1, 1)),
                          ("no nsites", (1, 1, 1, 0, 1)), ("no windows", (1, 1, 1, 1, 0)), ("maps only", (1, 1, 0, 0, 0))):
            d_start = torch.from_numpy(np.full((n_mo, codes.size), SENTINEL)).cuda()
            d_cover = torch.from_numpy(np.full((n_mo, codes.size), SENTINEL)).cuda()
            d_z = torch.full((len(keep), n_mo), -7.0, dtype=torch.float64, device="cuda")
            d_ns = torch.full((len(keep), n_mo), -7.0, dtype=torch.float64, device="cuda")
            d_win = torch.full((len(keep),), -7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            outs = [t.data_ptr() if a else None for t, a in zip((d_start, d_cover, d_z, d_ns, d_win), ask)]
            ctx.multisite_profile_dev(st, tabs, d_codes.data_ptr() if tabs is not None else None, d_prof.data_ptr(), dtype_code(dtype), codes.size,
                                      d_off.data_ptr(), d_len.data_ptr(), len(keep), d_lam.data_ptr(), *outs)
            ctx.synchronize()
            planes[name] = (d_start.cpu().numpy(), d_cover.cpu().numpy())
            for t, a, w in zip((d_z, d_ns, d_win), ask[2:], want[2:]):
                g = t.cpu().numpy()
                assert (rules.same_bits(g, w) if g.dtype == np.float64 else np.array_equal(g, w)) if a else (g == -7).all(), name
        for g, w in zip(planes["all"], want):
            assert is_sentinel(g[:, ~inside]).all() and not is_sentinel(g[:, inside]).any() and rules.same_bits(g[:, inside], w[:, inside])
        assert is_sentinel(planes["start"][1]).all() and is_sentinel(planes["cover"][0]).all()
        assert np.array_equal(planes["start"][0].view(np.uint64), planes["all"][0].view(np.uint64))
        assert np.array_equal(planes["cover"][1].view(np.uint64), planes["all"][1].view(np.uint64))
        for name in ("no z", "no nsites", "no windows", "maps only"):
            assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(planes[name], planes["all"])), name
    # one context, the family back to back: every call's buffers are its own or re-made
    ctx.stage(codes, profile)
    lam_all = lams(rng, len(off), 0.1)
    a = ctx.multisite_profile_staged(st, sq, off, lens, lam_all)
    o1 = ctx.occupancy_profile_staged(st, sq, off, lens)
    f1 = ctx.footprint_profile_staged(st, sq, 1, off, lens)
    m1 = ctx.multisite_staged(sq, None, off, lens, lam_all)
    b = ctx.multisite_profile_staged(st, sq, off, lens, lam_all)
    assert same(a, b) and same(a, want_of(codes, profile, off, lens, st, sq, lam_all))
    assert np.array_equal(o1[1], a[4]) and np.array_equal(f1[3], a[4]) and np.isfinite(m1[2]).all()
    assert (a[0][:, ~np.isin(np.arange(codes.size), np.concatenate([np.arange(o, o + n) for o, n in zip(off, lens)]))] == 0).all()   # +0.0 in _staged


def test_bad_arguments_launch_nothing(ctx):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(1231)
    codes, profile, off, lens = prules.stream(rng, [50, 60, 70], np.float32)
    lam = np.array([0.1, 0.2, 0.3])
    d_codes, d_prof = torch.from_numpy(codes).cuda(), torch.from_numpy(profile).cuda()
    d_off, d_len, d_lam = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(lam).cuda()
    d_start = torch.full((2, codes.size), -7.0, dtype=torch.float64, device="cuda")
    d_cover = torch.full((2, codes.size), -7.0, dtype=torch.float64, device="cuda")
    d_z = torch.full((3, 2), -7.0, dtype=torch.float64, device="cuda")
    d_key = torch.full((64,), -7, dtype=torch.int64, device="cuda")
    d_ev = torch.full((2, 64), -7.0, dtype=torch.float64, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L, h, p = ctx._L, ctx._h, _lib._ptr
    S = np.ascontiguousarray(np.stack([prules.struct_table(rng, 8)] * 2))
    R = np.ascontiguousarray(np.stack([orules.table(rng, 8, 4)] * 2))
    wide = np.ascontiguousarray(np.stack([prules.struct_table(rng, 65)] * 2))
    ptr = lambda t, shift=0: p(t.data_ptr() + shift) if t is not None else None

    def dev(st=S, sq=None, n_mo=2, m=8, c=d_codes, prof=d_prof, dt=_lib.PROFILE_F32, shift=0, shift_prof=0, n_pos=codes.size, o=d_off, ln=d_len,
            n_rec=3, la=d_lam, sta=d_start, cv=d_cover):
        return L.pfmscan_multisite_profile_dev(h, p(st), p(sq), n_mo, m, ptr(c, shift), ptr(prof, shift_prof), dt, n_pos, ptr(o), ptr(ln), n_rec,
                                               ptr(la), ptr(sta), ptr(cv), ptr(d_z), None, None)

    def events(thr=0.5, cap=64, key=d_key, cv=d_ev, n=d_n, la=d_lam, st=S):
        return L.pfmscan_multisite_profile_events_dev(h, p(st), None, 2, 8, None, ptr(d_prof), _lib.PROFILE_F32, codes.size, ptr(d_off), ptr(d_len), 3,
                                                      ptr(la), thr, cap, ptr(key), ptr(cv), ptr(cv, 64 * 8) if cv is not None else None, ptr(n),
                                                      None, None, None)
    assert dev(m=0) == _lib.E_BADSHAPE and dev(st=wide, m=65) == _lib.E_BADSHAPE
    assert dev(shift_prof=4) == _lib.E_BADSHAPE and dev(sq=R, shift=4) == _lib.E_BADSHAPE
    assert dev(dt=7) == _lib.E_BADARG
    assert dev(st=None) == _lib.E_BADARG and dev(st=None, sq=R) == _lib.E_BADARG        # struct_tables is required
    assert dev(la=None) == _lib.E_BADARG                                               # lam is required
    assert dev(sq=R, c=None) == _lib.E_BADARG                                          # joint mode needs the codes
    assert dev(prof=None) == _lib.E_BADARG and dev(o=None) == _lib.E_BADARG and dev(ln=None) == _lib.E_BADARG
    assert dev(sta=None, cv=None) == _lib.E_BADARG                                     # both planes NULL
    assert dev(n_pos=codes.size - 2) == _lib.E_BADARG and dev(n_mo=-1) == _lib.E_BADARG and dev(n_rec=-1) == _lib.E_BADARG
    swapped = torch.from_numpy(off[[1, 0, 2]].copy()).cuda()      # a bad record table: refused before a kernel forms an address
    torch.cuda.synchronize()
    assert dev(o=swapped) == _lib.E_BADARG
    assert dev(n_mo=0) == 0 and dev(n_rec=0) == 0
    assert events(thr=np.nan) == _lib.E_BADARG and events(key=None) == _lib.E_BADARG and events(cv=None) == _lib.E_BADARG
    assert events(n=None) == _lib.E_BADARG and events(cap=-1) == _lib.E_BADARG and events(la=None) == _lib.E_BADARG
    assert events(st=None) == _lib.E_BADARG
    ctx.synchronize()
    assert (d_start.cpu().numpy() == -7).all() and (d_cover.cpu().numpy() == -7).all() and (d_z.cpu().numpy() == -7).all()
    assert (d_key.cpu().numpy() == -7).all() and (d_ev.cpu().numpy() == -7).all() and int(d_n.cpu()[0]) == 0
    # structure only: the codes may be NULL and misaligned
    assert dev(c=None) == 0 and dev(shift=4) == 0
    ctx.synchronize()
    want = rules.multisite(profile, off, lens, S, None, None, lam, fill=-7.0)
    assert rules.same_bits(d_start.cpu().numpy(), want[0]) and rules.same_bits(d_cover.cpu().numpy(), want[1])
    assert rules.same_bits(d_z.cpu().numpy(), want[2])
    # the _staged form: what is staged, then the same checks
    ctx.stage(codes)
    with pytest.raises(ValueError):
        ctx.multisite_profile_staged(S, None, off, lens, lam)      # no profile staged
    ctx.stage(None, profile)
    with pytest.raises(ValueError):
        ctx.multisite_profile_staged(S, R, off, lens, lam)         # no codes staged
    ctx.stage(codes, profile)
    with pytest.raises(ValueError):
        ctx.multisite_profile_staged(S, R, off, lens, lam, want_start=False, want_cover=False)
    with pytest.raises(ValueError):
        ctx.multisite_profile_staged(wide, None, off, lens, lam)
    with pytest.raises(ValueError):
        ctx.multisite_profile_staged(S, R, off, lens, lam[:2])
    with pytest.raises(ValueError):
        ctx.multisite_profile_staged(S, R, off[[1, 0, 2]], lens, lam)
    k = ctypes.c_int64(-1)
    rc = L.pfmscan_multisite_profile_events_staged(h, None, None, 2, 8, p(off), p(lens), 3, p(lam), 0.5, 0, None, None, None, ctypes.byref(k), None,
                                                   None, None)
    assert rc == _lib.E_BADARG and k.value == -1
    rc = L.pfmscan_multisite_profile_staged(h, p(S), None, 2, 8, p(off), p(lens), 3, None, None, None, None, None, None)
    assert rc == _lib.E_BADARG


def test_engine_methods(ctx):
    from rnascan_amd import pack, scanner
    rng = np.random.default_rng(1283)
    e = scanner.HipEngine(0)
    try:
        lens = (5, 300, 0, 77)
        stream = pack.pack([rng.integers(0, 4, size=n).astype(np.uint8) for n in lens], [prules.rows(rng, n) for n in lens])
        st, sq = prules.struct_table(rng, 6), orules.table(rng, 6)
        lam = np.array([0.5, 0.01, 1.0, 0.05])
        ref = rules.RulesEngine()
        for tabs in (None, sq):
            want = ref.multisite_profile(stream, st, tabs, lam)
            assert same(e.multisite_profile(stream, st, tabs, lam), want)
            only = e.multisite_profile(stream, st, tabs, lam, want_cover=False)
            assert only[1] is None and rules.same_bits(only[0], want[0])
            thr = float(np.quantile(want[1], 0.9))
            got, wev = e.multisite_profile_events(stream, st, tabs, lam, thr), ref.multisite_profile_events(stream, st, tabs, lam, thr)
            assert np.array_equal(got[0], wev[0]) and all(rules.same_bits(g, w) for g, w in zip(got[1:5], wev[1:5])) and np.array_equal(got[5], wev[5])
    finally:
        e.close()
