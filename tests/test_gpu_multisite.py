"""The multi-site model (csrc/pfmscan_multisite.hip) on the GPU against the rules (tests/multisite_rules.py): every comparison
is on the float64 bit patterns (NaN == NaN), the int64 keys and Windows -- there is no tolerance in the contract."""
import ctypes

import numpy as np
import pytest

import multisite_rules as rules
import pair_rules as prules

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x7FF8DEAD0000BEEF], dtype=np.uint64).view(np.float64)[0]   # a NaN with a payload nothing computes
CAP_KNOB = "PFMSCAN_MULTISITE_SCRATCH_DOUBLES"
NAMES = ("start", "cover", "z", "nsites")


def tile_of(m):
    from rnascan_amd import _lib
    return _lib.MULTISITE_SLOTS - (m - 1)


def chunk():
    from rnascan_amd import _lib
    return _lib.MULTISITE_CHUNK


def stage(ctx, codes, codes2):
    ctx.stage(codes if codes is not None else codes2)
    if codes2 is not None:
        ctx.stage_codes2(codes2)


def run(ctx, codes, codes2, off, lens, R, S, lam, **kw):
    stage(ctx, codes, codes2)
    return ctx.multisite_staged(R, S, off, lens, lam, **kw)


def same(got, want):
    return (all(rules.same_bits(g, w) for g, w in zip(got[:4], want[:4])) and got[4].dtype == np.int64 and np.array_equal(got[4], want[4]))


def check(ctx, codes, codes2, off, lens, R, S, lam):
    got = run(ctx, codes, codes2, off, lens, R, S, lam)
    want = rules.multisite(codes, codes2, off, lens, R, S, lam)
    for name, g, w in zip(NAMES, got, want):
        assert rules.same_bits(g, w), "%s bits differ at %s" % (name, np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])
    assert got[4].dtype == np.int64 and np.array_equal(got[4], want[4])
    return got


def lams(rng, n, hi=0.5):
    lam = rng.uniform(0.0, hi, size=n)
    lam[::7] = 0.0                                                 # +0.0: Z = 1.0 and no site
    return lam


def ladder(rng, m):
    """every length 0 .. 3 m + 2, the lengths around the tile of the tile-parallel kernels and around the chunk of the serial
    ones (as windows and as positions), short records in between"""
    tile, c = tile_of(m), chunk()
    counts = [tile - 1, tile, tile + 1, 2 * tile + 1, c - 1, c, c + 1, 2 * c + m]
    around = [n + m - 1 for n in counts] + [tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1, c - 1, c, c + 1, 2 * c + m]
    lengths = list(range(0, 3 * m + 3))
    for x in around:
        lengths += [x, int(rng.integers(0, 2 * m + 2))]
    return lengths, counts


@pytest.mark.parametrize("m", [1, 2, 8, 12, 21, 64])
def test_length_ladder(ctx, m):
    rng = np.random.default_rng(900 + m)
    lengths, counts = ladder(rng, m)
    codes, off, lens = rules.stream(rng, lengths, 4, foreign=0.002)
    n_win = np.maximum(lens - m + 1, 0)
    for n in counts:
        assert (n_win == n).any() and (lens == n).any()
    for L in range(0, 3 * m + 3):
        assert (lens == L).any()
    R = rules.table(rng, m, 4, 0.6, 1.7)
    start, cover, z, ns, win = check(ctx, codes, None, off, lens, R, None, lams(rng, len(off)))
    assert not np.signbit(start).any() and not np.signbit(cover).any() and np.isfinite(z).all() and (z >= 1.0).all()
    for o, n, zz in zip(off, lens, z[:, 0]):                       # the record's last min(m - 1, L) starts, and the separator behind it
        assert (start[0, o + max(n - m + 1, 0):o + n + 1] == 0).all() and cover[0, o + n] == 0
        if n < m:
            assert zz == 1.0
        if n:
            assert cover[0, o:o + n].max() <= rules.cover_bound(int(n), m)
    o2, w2 = ctx.occupancy_staged(R, 4, off, lens, 0)              # Windows is the occupancy's count
    assert np.array_equal(w2, win)


def test_more_records_than_a_workgroup_retire_at_different_steps(ctx):
    rng = np.random.default_rng(901)
    m = 8
    lengths = [int(x) for x in rng.integers(0, 201, size=300)]
    lengths[40:40] = [5000, 0, 0]
    lengths[::31] = [0] * len(lengths[::31])
    codes, off, lens = rules.stream(rng, lengths, 4, foreign=0.002)
    assert len(off) > 256 and len(off) % 64 != 0
    Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(3)])
    check(ctx, codes, None, off, lens, Rs, None, lams(rng, len(off), 0.05))


@pytest.mark.parametrize("m", [1, 8, 21])
def test_foreign_codes(ctx, m):
    rng = np.random.default_rng(17 * m)
    L = 2 * m + 37
    codes, off, lens = rules.stream(rng, [L] * (L + 1) + [3 * m + 150, tile_of(m) + 3 * m])
    for p in range(L):                                             # record p: one foreign code at position p (every offset of a window)
        codes[off[p] + p] = np.uint8(rng.integers(4, 8))
    codes[off[L]:off[L] + L] = 7                                   # a record of nothing else
    codes[off[-2] + 60] = codes[off[-2] + 60 + max(m - 1, 1)] = 5  # two within m
    t = tile_of(m)
    codes[off[-1] + t - 1] = codes[off[-1] + t + m - 1] = 6        # on either side of a tile's edge
    R = rules.table(rng, m, 4)
    lam = rng.uniform(0.01, 0.3, size=len(off))
    start, cover, z, ns, win = check(ctx, codes, None, off, lens, R, None, lam)
    assert win[L] == 0 and z[L, 0] == 1.0 and ns[L, 0] == 0 and (cover[0, off[L]:off[L] + L] == 0).all()
    assert win[0] == L - m and win[L - 1] == L - m


def test_structure_letters_from_codes2(ctx):
    rng = np.random.default_rng(941)
    m = 9
    codes2, off, lens = rules.stream(rng, [int(x) for x in rng.integers(0, 900, size=40)] + [2 * tile_of(m) + 5], 7, foreign=0.003, case=True)
    assert (codes2 & 8).any()
    S = rules.table(rng, m, 7, 0.6, 1.7)
    lam = lams(rng, len(off), 0.1)
    got = check(ctx, None, codes2, off, lens, None, S, lam)
    plain = codes2.copy()
    plain[plain != 7] &= 7
    assert same(run(ctx, None, plain, off, lens, None, S, lam), got)
    noise = rng.integers(0, 8, size=codes2.size).astype(np.uint8)  # codes that are staged beside them are not read
    assert same(run(ctx, noise, codes2, off, lens, None, S, lam), got)


@pytest.mark.parametrize("m", [1, 8, 21])
def test_pairs_with_a_foreign_code_in_either_stream(ctx, m):
    rng = np.random.default_rng(7 * m + 3)
    L = 2 * m + 19
    codes, codes2, off, lens = prules.streams(rng, [L] * (2 * L) + [tile_of(m) + 2 * m, 0, 3], case=True)
    for p in range(L):
        codes[off[p] + p] = np.uint8(rng.integers(4, 8))
        codes2[off[L + p] + p] = np.uint8(7 | (8 if rng.random() < 0.3 else 0))
    codes2[off[-3] + tile_of(m)] = 7
    R, S = rules.table(rng, m, 4), rules.table(rng, m, 7)
    check(ctx, codes, codes2, off, lens, R, S, rng.uniform(0.01, 0.3, size=len(off)))


def test_passes_over_records_and_motifs_do_not_change_the_bits(ctx, monkeypatch):
    rng = np.random.default_rng(947)
    m = 12
    lengths = [int(x) for x in rng.integers(0, 700, size=40)] + [0, 1500]
    codes, codes2, off, lens = prules.streams(rng, lengths, foreign_seq=0.003, foreign_struct=0.003)
    Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(3)])
    Ss = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(3)])
    lam = lams(rng, len(off), 0.05)
    monkeypatch.delenv(CAP_KNOB, raising=False)
    for R, S in ((Rs, None), (Rs, Ss)):
        one = check(ctx, codes, codes2, off, lens, R, S, lam)
        stage(ctx, codes, codes2)
        want_ev = ctx.multisite_events_staged(R, S, off, lens, lam, 0.01)
        n_pos = codes.size
        # 2: every record and motif a pass of its own; n_pos / 2 positions: several passes over records, one motif each;
        # 4 n_pos: all records, two motifs then one
        for cap in (2, n_pos, 4 * n_pos + 8):
            monkeypatch.setenv(CAP_KNOB, str(cap))
            assert same(run(ctx, codes, codes2, off, lens, R, S, lam), one), cap
            ev = ctx.multisite_events_staged(R, S, off, lens, lam, 0.01)
            assert all(np.array_equal(np.asarray(g).view(np.uint64), np.asarray(w).view(np.uint64)) for g, w in zip(ev, want_ev)), cap
            monkeypatch.delenv(CAP_KNOB)


def test_independent_of_batch_and_place_in_the_stream(ctx):
    rng = np.random.default_rng(953)
    m = 12
    lengths = [int(x) for x in rng.integers(0, 900, size=30)] + [2 * tile_of(m) + 7]
    codes, codes2, off, lens = prules.streams(rng, lengths, foreign_seq=0.002, foreign_struct=0.002, case=True)
    Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(2)])
    Ss = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(2)])
    lam = lams(rng, len(off), 0.05)
    base = check(ctx, codes, codes2, off, lens, Rs, Ss, lam)
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

    want = dict(enumerate(per_record(base, off, lens)))
    shuffled = [int(i) for i in rng.permutation(len(recs))]
    for order, lead in ((list(range(13)), 0), (list(range(13, len(recs))), 3), (shuffled, 5), ([len(recs) - 1], 1)):
        c, c2, of, ln = packed(order, lead)
        got = run(ctx, c, c2, of, ln, Rs, Ss, lam[order])
        for i, (s, cv) in zip(order, per_record(got, of, ln)):
            assert rules.same_bits(s, want[i][0]) and rules.same_bits(cv, want[i][1])
        assert rules.same_bits(got[2], base[2][order]) and rules.same_bits(got[3], base[3][order]) and np.array_equal(got[4], base[4][order])
    # either map alone equals both together
    only_start = run(ctx, codes, codes2, off, lens, Rs, Ss, lam, want_cover=False)
    only_cover = run(ctx, codes, codes2, off, lens, Rs, Ss, lam, want_start=False)
    assert only_start[1] is None and only_cover[0] is None
    assert rules.same_bits(only_start[0], base[0]) and rules.same_bits(only_cover[1], base[1])
    assert rules.same_bits(only_start[2], base[2]) and rules.same_bits(only_cover[3], base[3])


def dev_maps(ctx, codes, codes2, off, lens, R, S, lam, want_start=True, want_cover=True, extras=False):
    """the _dev form on torch tensors, the planes pre-filled with the sentinel -> (start, cover[, z, nsites, windows])"""
    import torch
    T = np.asarray(R if R is not None else S)
    n_q = 1 if T.ndim == 2 else T.shape[0]
    n_pos = int((codes if codes is not None else codes2).size)
    d_codes = torch.from_numpy(codes).cuda() if codes is not None else None
    d_codes2 = torch.from_numpy(codes2).cuda() if codes2 is not None else None
    d_off, d_len = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).cuda(), torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int64)).cuda()
    d_lam = torch.from_numpy(np.ascontiguousarray(lam, dtype=np.float64)).cuda()
    d_start = torch.from_numpy(np.full((n_q, n_pos), SENTINEL)).cuda()
    d_cover = torch.from_numpy(np.full((n_q, n_pos), SENTINEL)).cuda()
    d_z = torch.full((len(off), n_q), -7.0, dtype=torch.float64, device="cuda")
    d_ns = torch.full((len(off), n_q), -7.0, dtype=torch.float64, device="cuda")
    d_win = torch.full((len(off),), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.multisite_dev(R, S, None if d_codes is None else d_codes.data_ptr(), None if d_codes2 is None else d_codes2.data_ptr(), n_pos,
                      d_off.data_ptr(), d_len.data_ptr(), len(off), d_lam.data_ptr(), d_start.data_ptr() if want_start else None,
                      d_cover.data_ptr() if want_cover else None, d_z.data_ptr() if extras else None, d_ns.data_ptr() if extras else None,
                      d_win.data_ptr() if extras else None)
    ctx.synchronize()
    out = (d_start.cpu().numpy(), d_cover.cpu().numpy())
    return out + (d_z.cpu().numpy(), d_ns.cpu().numpy(), d_win.cpu().numpy()) if extras else out


def is_sentinel(x):
    return np.asarray(x).view(np.uint64) == SENTINEL.view(np.uint64)


def test_dev_form_optional_outputs_and_special_values(ctx):
    rng = np.random.default_rng(967)
    m = 8
    codes, codes2, off, lens = prules.streams(rng, [int(x) for x in rng.integers(0, 700, size=24)] + [1100], foreign_seq=0.003, foreign_struct=0.003)
    codes[off[3]:off[3] + lens[3]] = 7                             # a record without a window with a term
    keep = np.array([i for i in range(len(off)) if i % 3 != 1])    # a table that skips records
    tables = []
    for kind in ("plain", "zero", "inf", "nan"):
        R = rules.table(rng, m, 4)
        if kind == "zero":
            R[0, :4] = 0.0
        if kind == "inf":
            R[m - 1, 2] = np.inf                                   # a +inf table cell
        if kind == "nan":
            R[m // 2, 0] = np.nan
        tables.append(R)
    Rs = np.stack(tables)
    S = np.stack([rules.table(rng, m, 7) for _ in tables])
    lam = lams(rng, len(keep), 0.2)
    lam[-1] = 1e6                                                  # 1100 positions at this activity: Z overflows
    inside = np.zeros(codes.size, dtype=bool)
    for o, n in zip(off[keep], lens[keep]):
        inside[o:o + n] = True
    for R_, S_ in ((Rs, None), (Rs, S)):
        want = rules.multisite(codes, codes2, off[keep], lens[keep], R_, S_, lam, fill=SENTINEL)
        assert not np.isfinite(want[2][-1, 0]) and want[2][0, 0] == 1.0 and np.isnan(want[2][:, 3]).any() and (want[2][:, 1] == 1.0).all()
        got = dev_maps(ctx, codes, codes2, off[keep], lens[keep], R_, S_, lam, extras=True)
        for g, w in zip(got[:2], want[:2]):
            assert is_sentinel(g[:, ~inside]).all() and not is_sentinel(g[:, inside]).any()
            assert rules.same_bits(g[:, inside], w[:, inside])
        assert rules.same_bits(got[2], want[2]) and rules.same_bits(got[3], want[3]) and np.array_equal(got[4], want[4])
        staged = run(ctx, codes, codes2, off[keep], lens[keep], R_, S_, lam)
        zero = rules.multisite(codes, codes2, off[keep], lens[keep], R_, S_, lam)
        assert same(staged, zero) and (staged[0][:, ~inside] == 0).all() and not np.signbit(staged[1][:, ~inside]).any()
        # one map alone: the same bits, the other plane untouched
        only_start = dev_maps(ctx, codes, codes2, off[keep], lens[keep], R_, S_, lam, want_cover=False)
        only_cover = dev_maps(ctx, codes, codes2, off[keep], lens[keep], R_, S_, lam, want_start=False)
        assert is_sentinel(only_start[1]).all() and is_sentinel(only_cover[0]).all()
        assert np.array_equal(only_start[0].view(np.uint64), got[0].view(np.uint64)) and np.array_equal(only_cover[1].view(np.uint64), got[1].view(np.uint64))


def raw_events(ctx, R, S, off, lens, lam, thr, cap, fill=-7):
    """pfmscan_multisite_events_staged as it stands -> (rc, n_events, key, cover, start), the arrays pre-filled"""
    from rnascan_amd import _lib
    sq, st = ctx._footprint_tables(R, S)
    n_q, m = (sq if sq is not None else st).shape[:2]
    off, lens = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(lens, dtype=np.int64)
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    key = np.full(max(cap, 1), fill, dtype=np.int64)
    cover, start = np.full(max(cap, 1), float(fill)), np.full(max(cap, 1), float(fill))
    k = ctypes.c_int64(-1)
    p = _lib._ptr
    rc = ctx._L.pfmscan_multisite_events_staged(ctx._h, p(sq), p(st), n_q, m, p(off), p(lens), off.size, p(lam), float(thr), cap, p(key), p(cover),
                                                p(start), ctypes.byref(k), None, None, None)
    return rc, int(k.value), key, cover, start


@pytest.mark.parametrize("pair", [False, True])
def test_events_are_the_filter_of_the_maps(ctx, pair):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(971 + pair)
    m = 12
    codes, codes2, off, lens = prules.streams(rng, [int(x) for x in rng.integers(0, 800, size=30)] + [0, 2 * tile_of(m) + 9],
                                              foreign_seq=0.002, foreign_struct=0.002)
    Rs = np.stack([rules.table(rng, m, 4, 0.3, 2.5) for _ in range(3)])
    Ss = np.stack([rules.table(rng, m, 7, 0.3, 2.5) for _ in range(3)]) if pair else None
    lam = rng.uniform(0.001, 0.02, size=len(off))
    start, cover, z, ns, win = rules.multisite(codes, codes2, off, lens, Rs, Ss, lam)
    inside = np.zeros(codes.size, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    sparse = float(np.quantile(cover[:, inside], 0.98))
    attained = float(np.sort(cover[0, inside])[int(0.9 * inside.sum())])
    stage(ctx, codes, codes2)
    for thr in (attained, np.nextafter(attained, -np.inf), -np.inf, sparse):
        want = rules.events(start, cover, off, lens, thr)
        got = ctx.multisite_events_staged(Rs, Ss, off, lens, lam, thr)
        assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]) and (np.diff(got[0]) > 0).all()
        assert rules.same_bits(got[1], want[1]) and rules.same_bits(got[2], want[2])
        assert rules.same_bits(got[3], z) and rules.same_bits(got[4], ns) and np.array_equal(got[5], win)
    at = int(np.flatnonzero((cover[0] == attained) & inside)[0])
    assert at not in set(rules.events(start, cover, off, lens, attained)[0].tolist())
    assert at in set(rules.events(start, cover, off, lens, np.nextafter(attained, -np.inf))[0].tolist())
    # a capacity one short: the verdict names the capacity that suffices and nothing was written
    want = rules.events(start, cover, off, lens, sparse)
    k = int(want[0].size)
    assert k > 10
    rc, n, key, cv, sw = raw_events(ctx, Rs, Ss, off, lens, lam, sparse, k - 1)
    assert rc == _lib.E_CAPACITY and n == k and (key == -7).all() and (cv == -7).all() and (sw == -7).all()
    rc, n, key, cv, sw = raw_events(ctx, Rs, Ss, off, lens, lam, sparse, k)
    assert rc == 0 and n == k and np.array_equal(key, want[0]) and rules.same_bits(cv, want[1]) and rules.same_bits(sw, want[2])
    with pytest.raises(_lib.CapacityError) as e:
        ctx.multisite_events_staged(Rs, Ss, off, lens, lam, sparse, capacity=k - 1)
    assert e.value.required == k
    got = ctx.multisite_events_staged(Rs, Ss, off, lens, lam, -np.inf)          # the default capacity is too small: one retry
    assert got[0].size == 3 * int(inside.sum()) > max(1024, codes.size // 16)
    rc, n, key, cv, sw = raw_events(ctx, Rs, Ss, off, lens, lam, np.nan, k)
    assert rc == _lib.E_BADARG and (key == -7).all()
    # the _dev form: unordered, the total in the counter, only the first `capacity` stored
    d_codes, d_codes2 = torch.from_numpy(codes).cuda(), torch.from_numpy(codes2).cuda()
    d_off, d_len, d_lam = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(lam).cuda()
    for cap in (k + 5, k // 2):
        d_key = torch.full((k + 5,), -7, dtype=torch.int64, device="cuda")
        d_cv = torch.full((k + 5,), -7.0, dtype=torch.float64, device="cuda")
        d_sw = torch.full((k + 5,), -7.0, dtype=torch.float64, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.multisite_events_dev(Rs, Ss, d_codes.data_ptr(), d_codes2.data_ptr() if pair else None, codes.size, d_off.data_ptr(), d_len.data_ptr(),
                                 len(off), d_lam.data_ptr(), sparse, cap, d_key.data_ptr(), d_cv.data_ptr(), d_sw.data_ptr(), d_n.data_ptr())
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
    rng = np.random.default_rng(977)
    codes, codes2, off, lens = prules.streams(rng, [50, 60, 70])
    lam = np.array([0.1, 0.2, 0.3])
    d_codes, d_codes2 = torch.from_numpy(codes).cuda(), torch.from_numpy(codes2).cuda()
    d_off, d_len, d_lam = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(lam).cuda()
    d_start = torch.full((2, codes.size), -7.0, dtype=torch.float64, device="cuda")
    d_cover = torch.full((2, codes.size), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L, h, p = ctx._L, ctx._h, _lib._ptr
    R, S = np.ascontiguousarray(np.stack([rules.table(rng, 8, 4)] * 2)), np.ascontiguousarray(np.stack([rules.table(rng, 8, 7)] * 2))
    wide = np.ascontiguousarray(np.stack([rules.table(rng, 65, 7)] * 2))
    ptr = lambda t, shift=0: p(t.data_ptr() + shift) if t is not None else None

    def dev(R=R, S=S, n_mo=2, m=8, c=d_codes, c2=d_codes2, shift=0, shift2=0, n_pos=codes.size, o=d_off, ln=d_len, n_rec=3, la=d_lam, st=d_start, cv=d_cover):
        return L.pfmscan_multisite_dev(h, p(R), p(S), n_mo, m, ptr(c, shift), ptr(c2, shift2), n_pos, ptr(o), ptr(ln), n_rec, ptr(la), ptr(st), ptr(cv),
                                       None, None, None)
    assert dev(m=0) == _lib.E_BADSHAPE and dev(R=wide, S=wide, m=65) == _lib.E_BADSHAPE
    assert dev(shift=4) == _lib.E_BADSHAPE and dev(shift2=8) == _lib.E_BADSHAPE
    assert dev(la=None) == _lib.E_BADARG and dev(R=None, S=None) == _lib.E_BADARG
    assert dev(c=None) == _lib.E_BADARG and dev(c2=None) == _lib.E_BADARG and dev(o=None) == _lib.E_BADARG
    assert dev(st=None, cv=None) == _lib.E_BADARG                           # both maps NULL
    assert dev(n_pos=codes.size - 2) == _lib.E_BADARG
    swapped = torch.from_numpy(off[[1, 0, 2]].copy()).cuda()               # a bad record table: refused before a kernel forms an address
    torch.cuda.synchronize()
    assert dev(o=swapped) == _lib.E_BADARG
    assert dev(n_mo=0) == 0 and dev(n_rec=0) == 0
    ctx.synchronize()
    assert (d_start.cpu().numpy() == -7).all() and (d_cover.cpu().numpy() == -7).all()
    assert dev(S=None, c2=None) == 0 and dev(R=None, c=None) == 0 and dev() == 0   # a stream that is not needed may be NULL
    ctx.synchronize()
    want = rules.multisite(codes, codes2, off, lens, R, S, lam, fill=-7.0)
    assert rules.same_bits(d_start.cpu().numpy(), want[0]) and rules.same_bits(d_cover.cpu().numpy(), want[1])
    ctx.stage(codes)
    with pytest.raises(ValueError):
        ctx.multisite_staged(R, S, off, lens, lam)                          # no codes2 staged
    ctx.stage_codes2(codes2)
    with pytest.raises(ValueError):
        ctx.multisite_staged(R, S, off, lens, lam, want_start=False, want_cover=False)
    with pytest.raises(ValueError):
        ctx.multisite_staged(R, S, off, lens, lam[:2])
    with pytest.raises(ValueError):
        ctx.multisite_staged(R, S, off[[1, 0, 2]], lens, lam)


def test_engine_methods(ctx):
    from rnascan_amd import pack, scanner
    rng = np.random.default_rng(983)
    e = scanner.HipEngine(0)
    try:
        lens = (5, 300, 0, 77)
        stream = pack.pack([rng.integers(0, 4, size=n).astype(np.uint8) for n in lens])
        letters = pack.pack([rng.integers(0, 7, size=n).astype(np.uint8) for n in lens])   # a structure-letter FASTA on its own: codes, no codes2
        R, S = rules.table(rng, 6, 4), rules.table(rng, 6, 7)
        lam = np.array([0.5, 0.01, 1.0, 0.05])
        ref = rules.RulesEngine()
        assert same(e.multisite(letters, None, S, lam), ref.multisite(letters, None, S, lam))
        assert same(e.multisite(stream, R, None, lam), ref.multisite(stream, R, None, lam))
        stream.codes2 = letters.codes
        want = ref.multisite(stream, R, S, lam)
        assert same(e.multisite(stream, R, S, lam), want)
        thr = float(np.quantile(want[1], 0.9))
        got, wev = e.multisite_events(stream, R, S, lam, thr), ref.multisite_events(stream, R, S, lam, thr)
        assert np.array_equal(got[0], wev[0]) and all(rules.same_bits(g, w) for g, w in zip(got[1:5], wev[1:5])) and np.array_equal(got[5], wev[5])
    finally:
        e.close()
