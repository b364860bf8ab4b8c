"""The threshold-free mutagenesis (k_mutocc / k_mutocc_rolled, csrc/pfmscan_mutocc.hip) on the GPU against the rules
(tests/mutocc_rules.py): every comparison is on the float64 bit patterns (NaN == NaN), the int64 keys and Windows -- there is
no tolerance in the contract."""
import ctypes
import functools
import io
import os

import numpy as np
import pytest

import footprint_rules as frules
import mutocc_rules as rules
from conftest import DATA_DIR, REPO

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x7FF8DEAD0000BEEF], dtype=np.uint64).view(np.float64)[0]   # a NaN with a payload nothing computes
FIXED_MAX = 20                                                     # the widest compile-time width (MO_FIXED_MAX)
WIDTHS = [1, 2, 8, 12, FIXED_MAX, FIXED_MAX + 1, 64]
FIXTURE = os.path.join(REPO, "tests", "golden", "variant_occupancy", "hist_slbp_saturate.tsv")
FIXTURE_ARGV = ["-p", os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt"), "-u", "-C", "0", "--saturate",
                os.path.join(DATA_DIR, "HIST2H3C_3p_end.fa")]


def tile():
    from rnascan_amd import _lib
    return _lib.MUTOCC_TILE


@functools.lru_cache(maxsize=None)
def case(m):
    """one stream per width: positions with fewer than m windows at both ends of a record, halos across a tile's edge on both
    sides; 2 % foreign codes, the case bit on a third of the letters; three tables -> (codes, off, lens, tables, the rules' answer)"""
    rng = np.random.default_rng(900 + m)
    t = tile()
    lengths = [0, 1, m - 1, m, m + 1, 2 * m - 1, 2 * m, t - 1, t, t + 1, t + m, 2 * t + 5]
    codes, off, lens = rules.stream(rng, lengths, 4, foreign=0.02, case=True)
    codes[off[-1] + t - 1] = codes[off[-1] + 2 * t] = 6            # on either side of a tile's edge
    assert (codes & 8).any()
    Rs = np.stack([rules.table(rng, m, 4, 0.3, 2.5) for _ in range(3)])
    for a in (codes, off, lens, Rs):
        a.setflags(write=False)
    return codes, off, lens, Rs, rules.mutocc(codes, off, lens, Rs)


def same(got, want):
    return (rules.same_bits(got[0], want[0]) and rules.same_bits(got[1], want[1]) and got[2].dtype == np.int64 and np.array_equal(got[2], want[2]))


@pytest.mark.parametrize("m", WIDTHS)
def test_the_map_on_the_length_ladder(ctx, m, monkeypatch):
    codes, off, lens, Rs, want = case(m)
    ctx.stage(codes)
    got = ctx.mutocc_staged(Rs, off, lens)
    for name, g, w in zip(("local", "occ"), got, want):
        assert rules.same_bits(g, w), "%s bits differ at %s" % (name, np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])
    assert got[2].dtype == np.int64 and np.array_equal(got[2], want[2])
    # one motif alone: the same bits
    one = ctx.mutocc_staged(Rs[1], off, lens)
    assert same(one, (want[0][1:2], want[1][:, 1:2], want[2]))
    # the rolled form gives the compile-time form's bits
    monkeypatch.setenv("PFMSCAN_MUTOCC_ROLLED", "1")
    assert same(ctx.mutocc_staged(Rs, off, lens), want)
    monkeypatch.delenv("PFMSCAN_MUTOCC_ROLLED")
    # the shipped siblings: the ref column is the posterior site map's ratio cover, occ and windows are the occupancy's
    _, cover, occ, win = ctx.footprint_staged(Rs, None, frules.RATIO, off, lens, want_start=False)
    c = codes & 7
    inside = np.zeros(codes.size, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    p = np.flatnonzero(inside & (c < 4))
    for q in range(3):
        assert rules.same_bits(got[0][q, p, c[p]], cover[q, p])
    assert np.isnan(got[0][:, ~(inside & (c < 4))]).all() and not np.isnan(got[0][:, p]).any()
    o2, w2 = ctx.occupancy_staged(Rs, 4, off, lens, 0)
    assert rules.same_bits(got[1], occ) and rules.same_bits(got[1], o2) and np.array_equal(got[2], win) and np.array_equal(got[2], w2)


def test_special_tables(ctx):
    rng = np.random.default_rng(61)
    m = 8
    codes, off, lens = rules.stream(rng, [0, 5, 40, 333, tile() + 9], 4, foreign=0.02)
    zero, inf = rules.table(rng, m), rules.table(rng, m)
    zero[3, 1] = 0.0
    inf[2, 2] = np.inf
    inf[5, 0] = 0.0                                                # 0 * inf where both meet
    Rs = np.stack([zero, inf])
    ctx.stage(codes)
    got = ctx.mutocc_staged(Rs, off, lens)
    want = rules.mutocc(codes, off, lens, Rs)
    assert same(got, want)
    assert (got[0][0] == 0).any() and np.isinf(got[0][1]).any()


def dev_map(ctx, codes, off, lens, Rs):
    """the _dev form on torch tensors, the map pre-filled with the sentinel -> local as it lies on the device"""
    import torch
    d_codes = torch.from_numpy(np.array(codes)).cuda()
    d_off, d_len = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).cuda(), torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int64)).cuda()
    d_local = torch.from_numpy(np.full((Rs.shape[0], codes.size, 4), SENTINEL)).cuda()
    torch.cuda.synchronize()
    ctx.mutocc_dev(Rs, d_codes.data_ptr(), codes.size, d_off.data_ptr(), d_len.data_ptr(), len(off), d_local.data_ptr())
    ctx.synchronize()
    return d_local.cpu().numpy()


def test_the_dev_form_writes_inside_the_records_only(ctx):
    m = 12
    codes, off, lens, Rs, _ = case(m)
    keep = np.array([i for i in range(len(off)) if i % 3 != 1])    # a table that skips records
    got = dev_map(ctx, codes, off[keep], lens[keep], Rs)
    want = rules.mutocc(codes, off[keep], lens[keep], Rs, fill=SENTINEL)[0]
    inside = np.zeros(codes.size, dtype=bool)
    for o, n in zip(off[keep], lens[keep]):
        inside[o:o + n] = True
    untouched = got.view(np.uint64) == SENTINEL.view(np.uint64)
    assert untouched[:, ~inside].all() and not untouched[:, inside].any()
    assert rules.same_bits(got[:, inside], want[:, inside])


def raw_events(ctx, Rs, off, lens, frac, cap, fill=-7):
    """pfmscan_mutocc_events_staged as it stands -> (rc, n_events, key, alt, ref), the arrays pre-filled"""
    from rnascan_amd import _lib
    T = np.ascontiguousarray(Rs, dtype=np.float64)
    off, lens = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(lens, dtype=np.int64)
    key = np.full(max(cap, 1), fill, dtype=np.int64)
    alt, ref = np.full(max(cap, 1), float(fill)), np.full(max(cap, 1), float(fill))
    k = ctypes.c_int64(-1)
    p = _lib._ptr
    rc = ctx._L.pfmscan_mutocc_events_staged(ctx._h, p(T), T.shape[0], T.shape[1], p(off), p(lens), off.size, float(frac), cap, p(key), p(alt), p(ref),
                                             ctypes.byref(k), None, None)
    return rc, int(k.value), key, alt, ref


@pytest.mark.parametrize("m", [8, FIXED_MAX + 1])
def test_events_are_the_filter_of_the_map(ctx, m):
    import torch
    from rnascan_amd import _lib
    codes, off, lens, Rs, (local, occ, win) = case(m)
    ctx.stage(codes)
    sizes = {}
    for frac in (0.0, 0.5):
        want = rules.events(local, codes, off, lens, occ, frac)
        got = ctx.mutocc_events_staged(Rs, off, lens, frac)
        assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]) and (np.diff(got[0]) > 0).all()
        assert rules.same_bits(got[1], want[1]) and rules.same_bits(got[2], want[2])
        assert rules.same_bits(got[3], occ) and np.array_equal(got[4], win)
        sizes[frac] = int(want[0].size)
    assert sizes[0.0] > sizes[0.5] > 0
    # a capacity one short: the verdict names the capacity that suffices and nothing was written
    want = rules.events(local, codes, off, lens, occ, 0.5)
    k = sizes[0.5]
    rc, n, key, alt, ref = raw_events(ctx, Rs, off, lens, 0.5, k - 1)
    assert rc == _lib.E_CAPACITY and n == k and (key == -7).all() and (alt == -7).all() and (ref == -7).all()
    rc, n, key, alt, ref = raw_events(ctx, Rs, off, lens, 0.5, k)
    assert rc == 0 and n == k and np.array_equal(key, want[0]) and rules.same_bits(alt, want[1]) and rules.same_bits(ref, want[2])
    with pytest.raises(_lib.CapacityError) as e:
        ctx.mutocc_events_staged(Rs, off, lens, 0.5, capacity=k - 1)
    assert e.value.required == k
    for bad in (np.nan, -0.5):
        rc, n, key, alt, ref = raw_events(ctx, Rs, off, lens, bad, k)
        assert rc == _lib.E_BADARG and (key == -7).all()
    # the _dev form: unordered, the total in the counter, only the first `capacity` stored
    d_codes = torch.from_numpy(np.array(codes)).cuda()
    d_off, d_len = torch.from_numpy(np.array(off)).cuda(), torch.from_numpy(np.array(lens)).cuda()
    for cap in (k + 5, k // 2):
        d_key = torch.full((k + 5,), -7, dtype=torch.int64, device="cuda")
        d_alt = torch.full((k + 5,), -7.0, dtype=torch.float64, device="cuda")
        d_ref = torch.full((k + 5,), -7.0, dtype=torch.float64, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.mutocc_events_dev(Rs, d_codes.data_ptr(), codes.size, d_off.data_ptr(), d_len.data_ptr(), len(off), 0.5, cap, d_key.data_ptr(),
                              d_alt.data_ptr(), d_ref.data_ptr(), d_n.data_ptr())
        ctx.synchronize()
        assert int(d_n.cpu()[0]) == k
        key, alt, ref = d_key.cpu().numpy(), d_alt.cpu().numpy(), d_ref.cpu().numpy()
        stored = min(cap, k)
        assert (key[stored:] == -7).all() and (alt[stored:] == -7).all() and (ref[stored:] == -7).all()
        order = np.argsort(key[:stored])
        where = np.searchsorted(want[0], key[:stored][order])
        assert np.array_equal(want[0][where], key[:stored][order]) and (np.diff(key[:stored][order]) > 0).all()
        assert rules.same_bits(alt[:stored][order], want[1][where]) and rules.same_bits(ref[:stored][order], want[2][where])


def test_error_paths_write_nothing(ctx):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(67)
    codes, off, lens = rules.stream(rng, [50, 60, 70])
    d_codes = torch.from_numpy(codes).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    d_local = torch.full((2, codes.size, 4), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L, h, p = ctx._L, ctx._h, _lib._ptr
    R = np.ascontiguousarray(np.stack([rules.table(rng, 8, 4)] * 2))
    wide = np.ascontiguousarray(np.stack([rules.table(rng, 65, 4)] * 2))
    ptr = lambda t, shift=0: p(t.data_ptr() + shift) if t is not None else None

    def dev(R=R, n_mo=2, m=8, c=d_codes, shift=0, n_pos=codes.size, o=d_off, ln=d_len, n_rec=3, lo=d_local, lshift=0):
        return L.pfmscan_mutocc_dev(h, p(R), n_mo, m, ptr(c, shift), n_pos, ptr(o), ptr(ln), n_rec, ptr(lo, lshift), None, None)
    assert dev(m=0) == _lib.E_BADSHAPE and dev(R=wide, m=65) == _lib.E_BADSHAPE
    assert dev(shift=4) == _lib.E_BADSHAPE and dev(lshift=8) == _lib.E_BADSHAPE
    assert dev(R=None) == _lib.E_BADARG and dev(c=None) == _lib.E_BADARG and dev(o=None) == _lib.E_BADARG and dev(lo=None) == _lib.E_BADARG
    assert dev(n_pos=codes.size - 2) == _lib.E_BADARG
    swapped = torch.from_numpy(off[[1, 0, 2]].copy()).cuda()               # a bad record table: refused before a kernel forms an address
    torch.cuda.synchronize()
    assert dev(o=swapped) == _lib.E_BADARG
    assert dev(n_mo=0) == 0 and dev(n_rec=0) == 0
    ctx.synchronize()
    assert (d_local.cpu().numpy() == -7).all()
    assert dev() == 0
    ctx.synchronize()
    assert rules.same_bits(d_local.cpu().numpy(), rules.mutocc(codes, off, lens, R, fill=-7.0)[0])
    ctx.stage(codes)
    with pytest.raises(ValueError):
        ctx.mutocc_staged(wide, off, lens)
    with pytest.raises(ValueError):
        ctx.mutocc_staged(R, off[[1, 0, 2]], lens)


def test_engine_methods_and_the_command_on_the_device(ctx):
    from rnascan_amd import pack, scanner, variant_occupancy
    rng = np.random.default_rng(71)
    e = scanner.HipEngine(0)
    try:
        stream = pack.pack([rng.integers(0, 4, size=n).astype(np.uint8) for n in (5, 300, 0, 77)])
        R = rules.table(rng, 6, 4, 0.2, 4.0)
        ref = rules.RulesEngine()
        assert same(e.mutocc(stream, R), ref.mutocc(stream, R))
        for capacity in (None, 4000):
            got, want = e.mutocc_events(stream, R, 0.05, capacity), ref.mutocc_events(stream, R, 0.05)
            assert want[0].size and np.array_equal(got[0], want[0]) and rules.same_bits(got[1], want[1]) and rules.same_bits(got[2], want[2])
        # a capacity verdict is answered by growing: the default capacity is far below 3 events per position at frac 0
        long = pack.pack([rng.integers(0, 4, size=9000).astype(np.uint8)])
        got, want = e.mutocc_events(long, R, 0.0), ref.mutocc_events(long, R, 0.0)
        assert want[0].size > 9000 and np.array_equal(got[0], want[0]) and rules.same_bits(got[1], want[1])
        # the command: the committed fixture byte for byte, whatever the batch size
        for extra in ([], ["--batch-records", "1"]):
            out = io.StringIO()
            assert variant_occupancy.main(FIXTURE_ARGV + extra, engine=e, out=out) == 0
            assert out.getvalue() == open(FIXTURE).read()
    finally:
        e.close()
