"""The occupancy of two code streams (k_occ_blocks<QN, true>, csrc/pfmscan_occupancy.hip) on the GPU against the rules
(tests/pair_rules.py): every comparison is on the float64 bit patterns (NaN == NaN) plus equal Windows -- there is no
tolerance in the contract."""
import numpy as np
import pytest

import pair_rules as rules
from test_gpu_occupancy import length_ladder

pytestmark = pytest.mark.gpu


def run(ctx, codes, codes2, off, lens, R, S):
    ctx.stage(codes)
    ctx.stage_codes2(codes2)
    return ctx.occupancy_pair_staged(R, S, off, lens)


def same(got, want):
    return rules.same_bits(got[0], want[0]) and got[1].dtype == np.int64 and np.array_equal(got[1], want[1])


def check(ctx, codes, codes2, off, lens, R, S):
    got = run(ctx, codes, codes2, off, lens, R, S)
    want = rules.occupancy(codes, codes2, off, lens, R, S)
    assert same(got, want), "occupancy bits differ at %s" % np.argwhere(~((got[0] == want[0]) | (np.isnan(got[0]) & np.isnan(want[0]))))[:5]
    return got


@pytest.mark.parametrize("m", [1, 2, 8, 12, 21, 64])
def test_record_lengths_and_widths(ctx, m):
    rng = np.random.default_rng(200 + m)
    codes, codes2, off, lens = rules.streams(rng, length_ladder(rng, m), foreign_seq=0.001, foreign_struct=0.001, case=True)
    R, S = rules.table(rng, m, 4, 0.6, 1.7), rules.table(rng, m, 7, 0.6, 1.7)
    got = check(ctx, codes, codes2, off, lens, R, S)
    n_win = np.maximum(lens - m + 1, 0)
    for n in (0, 1, 31, 32, 33, 1023, 1024, 1025, 32768, 32769):
        assert (n_win == n).any()
    assert (got[0][n_win == 0] == 0).all() and not np.signbit(got[0][n_win == 0]).any() and (got[1][n_win == 0] == 0).all()
    assert np.isfinite(got[0]).all() and (got[0][got[1] > 0] > 0).all()


@pytest.mark.parametrize("m", [1, 8, 21, 64])
def test_foreign_codes_in_either_stream(ctx, m):
    """a foreign code in the sequence stream only, in the structure stream only and in both: at a record's first and last
    position, at every offset of one window, two within m of each other; a third of the structure letters carry bit 3 and
    count as their letter; a record that is foreign throughout in one stream"""
    rng = np.random.default_rng(7 * m)
    L = 2 * m + 37
    n_each = L + 2 * m + 2
    codes, codes2, off, lens = rules.streams(rng, [L] * (3 * n_each) + [5 * m + 200] * 3, case=True)
    bad1 = lambda: np.uint8(rng.integers(4, 8))
    bad2 = lambda: np.uint8(7 | (8 if rng.random() < 0.3 else 0))
    for which in range(3):                                            # 0: sequence only, 1: structure only, 2: both
        base = which * n_each

        def put(r, p):
            if which in (0, 2):
                codes[off[r] + p] = bad1()
            if which in (1, 2):
                codes2[off[r] + p] = bad2()
        for p in range(L):                                             # record p: one foreign code at position p
            put(base + p, p)
        for d in range(1, 2 * m + 1):                                  # two of them d apart (within m and beyond)
            put(base + L + d, 10)
            put(base + L + d, min(10 + d, L - 1))
        r = base + L + 2 * m + 1                                       # nothing but foreign codes, in the stream(s) of this part
        if which in (0, 2):
            codes[off[r]:off[r] + L] = 7
        if which in (1, 2):
            codes2[off[r]:off[r] + L] = 7
    codes[off[-1] + 100:off[-1] + 100 + m + 3] = 7
    codes2[off[-2] + 50:off[-2] + 50 + m + 3] = 7
    R, S = rules.table(rng, m, 4), rules.table(rng, m, 7)
    got = check(ctx, codes, codes2, off, lens, R, S)
    for which in range(3):
        base = which * n_each
        r = base + L + 2 * m + 1
        assert got[1][r] == 0 and got[0][r, 0] == 0 and not np.signbit(got[0][r, 0])
        assert got[1][base] == L - m + 1 - 1 and got[1][base + L - 1] == L - m + 1 - 1      # the first and the last position lie in one window each
    plain = codes2.copy()
    plain[plain != 7] &= 7
    assert (plain != codes2).any()
    assert same(run(ctx, codes, plain, off, lens, R, S), got)


def test_special_cells(ctx):
    """+0.0, +inf and NaN in either table, 0 x inf across the two chains; products that go subnormal and to 0, and overflow"""
    rng = np.random.default_rng(3)
    lens = [int(x) for x in rng.integers(1, 400, size=60)] + [3000]
    for m in (2, 8, 64):
        codes, codes2, off, ln = rules.streams(rng, [x + m - 1 for x in lens], foreign_seq=0.005, foreign_struct=0.005)
        Rs, Ss = [], []
        for kind in ("zero_seq", "zero_struct", "inf_seq", "inf_struct", "nan_seq", "nan_struct", "zero_x_inf", "inf_x_zero"):
            R, S = rules.table(rng, m, 4), rules.table(rng, m, 7)
            if kind == "zero_seq":
                R[0, 1] = 0.0
            if kind == "zero_struct":
                S[m - 1, 4] = 0.0
            if kind == "inf_seq":
                R[m - 1, 2] = np.inf
            if kind == "inf_struct":
                S[0, 3] = np.inf
            if kind == "nan_seq":
                R[m // 2, 0] = np.nan
            if kind == "nan_struct":
                S[m // 2, 6] = np.nan
            if kind == "zero_x_inf":
                R[0, :4], S[m - 1, :7] = 0.0, np.inf                   # the letters reach +0.0, the structure multiplies by +inf
            if kind == "inf_x_zero":
                R[m - 1, :4], S[0, :7] = np.inf, 0.0
            Rs.append(R)
            Ss.append(S)
        small_r, small_s = np.full((m, 8), np.nan), np.full((m, 8), np.nan)
        small_r[:, :4] = rng.choice([1e-3, 1e-2, 2e-3], size=(m, 4))
        small_s[:, :7] = rng.choice([1e-3, 1e-2, 2e-3], size=(m, 7))
        large_r, large_s = np.full((m, 8), np.nan), np.full((m, 8), np.nan)
        large_r[:, :4] = rng.choice([1e2, 1e3, 7e2], size=(m, 4))
        large_s[:, :7] = rng.choice([1e2, 1e3, 7e2], size=(m, 7))
        Rs += [small_r, large_r]
        Ss += [small_s, large_s]
        got = check(ctx, codes, codes2, off, ln, np.stack(Rs), np.stack(Ss))[0]
        assert np.isposinf(got[-1, 2]) and np.isposinf(got[-1, 3]) and np.isnan(got[-1, 4]) and np.isnan(got[-1, 5])
        assert np.isnan(got[-1, 6]) and np.isnan(got[-1, 7])
        if m == 64:
            t, _ = rules.terms(codes, codes2, off[-1], ln[-1], small_r, small_s)
            assert ((t > 0) & (t < 2.3e-308)).any() and (t == 0).any()
            assert np.isposinf(got[:, 9]).any()


def test_libraries_across_the_lds_chunk_rule(ctx):
    """chunk - 1, chunk, chunk + 1 and 2 chunk + 3 pairs at m = 12, and a few small libraries: pair k's column is the
    single-pair call on tables k"""
    rng = np.random.default_rng(11)
    m = 12
    chunk = rules.lds_chunk(m)
    assert chunk == 8
    codes, codes2, off, lens = rules.streams(rng, [int(x) for x in rng.integers(1, 300, size=40)] + [2500], foreign_seq=0.01, foreign_struct=0.01, case=True)
    n_max = 2 * chunk + 3
    Rs = np.stack([rules.table(rng, m, 4) for _ in range(n_max)])
    Ss = np.stack([rules.table(rng, m, 7) for _ in range(n_max)])
    want = rules.occupancy(codes, codes2, off, lens, Rs, Ss)
    ctx.stage(codes)
    ctx.stage_codes2(codes2)
    single = {}
    for n in (1, 2, 3, 5, chunk - 1, chunk, chunk + 1, n_max):
        occ, win = ctx.occupancy_pair_staged(Rs[:n], Ss[:n], off, lens)
        assert rules.same_bits(occ, want[0][:, :n]) and np.array_equal(win, want[1])
        for k in (0, n // 2, n - 1):
            if k not in single:
                single[k] = ctx.occupancy_pair_staged(Rs[k], Ss[k], off, lens)[0][:, 0]
            assert rules.same_bits(occ[:, k], single[k])
    # the widest pair: a chunk holds two
    m = 64
    assert rules.lds_chunk(m) == 2
    codes, codes2, off, lens = rules.streams(rng, [int(x) + m for x in rng.integers(1, 300, size=20)], foreign_seq=0.002, foreign_struct=0.002)
    Rs = np.stack([rules.table(rng, m, 4, 0.7, 1.5) for _ in range(5)])
    Ss = np.stack([rules.table(rng, m, 7, 0.7, 1.5) for _ in range(5)])
    check(ctx, codes, codes2, off, lens, Rs, Ss)


def test_scratch_passes_change_no_bit(ctx, monkeypatch):
    rng = np.random.default_rng(13)
    m = 12
    codes, codes2, off, lens = rules.streams(rng, [int(x) for x in rng.integers(1, 1500, size=50)] + [40000] + [int(x) for x in rng.integers(1, 200, size=20)],
                                             foreign_seq=0.003, foreign_struct=0.003)
    Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(7)])
    Ss = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(7)])
    want = check(ctx, codes, codes2, off, lens, Rs, Ss)
    for cap in ("1", "50", "3000", "100000"):
        monkeypatch.setenv("PFMSCAN_OCC_SCRATCH_DOUBLES", cap)
        assert same(run(ctx, codes, codes2, off, lens, Rs, Ss), want)


def test_independent_of_order_batch_and_stream_offset(ctx):
    """the same records shuffled, split into two batches, and placed at stream offsets 0 .. 3 mod 4: the same per-record bits"""
    rng = np.random.default_rng(17)
    m = 12
    lengths = [int(x) for x in rng.integers(1, 4000, size=80)] + [33000]
    codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.002, foreign_struct=0.002, case=True)
    Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(3)])
    Ss = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(3)])
    base = check(ctx, codes, codes2, off, lens, Rs, Ss)
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

    order = rng.permutation(len(recs))
    got = run(ctx, *packed(order), Rs, Ss)
    assert rules.same_bits(got[0], base[0][order]) and np.array_equal(got[1], base[1][order])
    cut = 37
    a = run(ctx, *packed(range(cut)), Rs, Ss)
    b = run(ctx, *packed(range(cut, len(recs))), Rs, Ss)
    assert rules.same_bits(np.concatenate([a[0], b[0]]), base[0]) and np.array_equal(np.concatenate([a[1], b[1]]), base[1])
    for lead in (1, 2, 3):
        assert same(run(ctx, *packed(range(len(recs)), lead), Rs, Ss), base)
    some = np.sort(rng.choice(len(recs), size=20, replace=False))
    ctx.stage(codes)
    ctx.stage_codes2(codes2)
    part = ctx.occupancy_pair_staged(Rs, Ss, off[some], lens[some])
    assert rules.same_bits(part[0], base[0][some]) and np.array_equal(part[1], base[1][some])


def test_identities_against_the_single_stream_entry_points(ctx):
    rng = np.random.default_rng(19)
    for m in (8, 21):
        lengths = [int(x) + m - 1 for x in rng.integers(1, 3000, size=40)] + [m - 1, 33000]
        Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(9)])
        Ss = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(9)])
        one = np.stack([rules.ones(m)] * 9)
        codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.004, foreign_struct=0.0, case=True)
        got = run(ctx, codes, codes2, off, lens, Rs, one)
        assert same(got, ctx.occupancy_staged(Rs, 4, off, lens, 0))
        codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.0, foreign_struct=0.004, case=True)
        got = run(ctx, codes, codes2, off, lens, one, Ss)
        assert same(got, ctx.occupancy_staged(Ss, 7, off, lens, 1))


def test_engine_method(ctx):
    from rnascan_amd import pack, scanner
    rng = np.random.default_rng(23)
    e = scanner.HipEngine(0)
    try:
        lens = (5, 300, 0, 77)
        stream = pack.pack([rng.integers(0, 4, size=n).astype(np.uint8) for n in lens])
        stream.codes2 = pack.pack([rng.integers(0, 7, size=n).astype(np.uint8) for n in lens]).codes
        R, S = rules.table(rng, 6, 4), rules.table(rng, 6, 7)
        got = e.occupancy_pair(stream, R, S)
        assert same(got, rules.occupancy(stream.codes, stream.codes2, stream.offsets, stream.lengths, R, S))
        assert same(e.occupancy_pair(stream, R[None], S[None]), got)
    finally:
        e.close()


def test_dev_form_as_an_integrator_calls_it(ctx):
    """torch device tensors in and out on the context's stream; equal to _staged; nothing written outside the outputs"""
    import torch
    rng = np.random.default_rng(29)
    m, n_mo = 12, 5
    codes, codes2, off, lens = rules.streams(rng, [int(x) for x in rng.integers(1, 2000, size=60)], foreign_seq=0.003, foreign_struct=0.003, case=True)
    Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(n_mo)])
    Ss = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(n_mo)])
    want = check(ctx, codes, codes2, off, lens, Rs, Ss)
    n_rec, guard = len(off), 64
    d_codes, d_codes2 = torch.from_numpy(codes).cuda(), torch.from_numpy(codes2).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    d_occ = torch.full((guard + n_rec * n_mo + guard,), -7.0, dtype=torch.float64, device="cuda")
    d_win = torch.full((guard + n_rec + guard,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.occupancy_pair_dev(Rs, Ss, d_codes.data_ptr(), d_codes2.data_ptr(), codes.size, d_off.data_ptr(), d_len.data_ptr(), n_rec,
                           d_occ.data_ptr() + 8 * guard, d_win.data_ptr() + 8 * guard)
    ctx.synchronize()
    occ, win = d_occ.cpu().numpy(), d_win.cpu().numpy()
    assert (occ[:guard] == -7).all() and (occ[-guard:] == -7).all() and (win[:guard] == -7).all() and (win[-guard:] == -7).all()
    assert rules.same_bits(occ[guard:-guard].reshape(n_rec, n_mo), want[0]) and np.array_equal(win[guard:-guard], want[1])
    d_occ.fill_(-7.0)
    torch.cuda.synchronize()
    ctx.occupancy_pair_dev(Rs, Ss, d_codes.data_ptr(), d_codes2.data_ptr(), codes.size, d_off.data_ptr(), d_len.data_ptr(), n_rec,
                           d_occ.data_ptr() + 8 * guard, None)
    ctx.synchronize()
    assert rules.same_bits(d_occ.cpu().numpy()[guard:-guard].reshape(n_rec, n_mo), want[0])


def test_bad_arguments_launch_nothing(ctx):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(31)
    codes, codes2, off, lens = rules.streams(rng, [50, 60, 70])
    d_codes, d_codes2 = torch.from_numpy(codes).cuda(), torch.from_numpy(codes2).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    d_occ = torch.full((3, 2), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L, h, p = ctx._L, ctx._h, _lib._ptr
    R, S = np.ascontiguousarray(np.stack([rules.table(rng, 8, 4)] * 2)), np.ascontiguousarray(np.stack([rules.table(rng, 8, 7)] * 2))
    wide = np.ascontiguousarray(np.stack([rules.table(rng, 65, 7)] * 2))
    ptr = lambda t, shift=0: p(t.data_ptr() + shift) if t is not None else None

    def dev(R=R, S=S, n_mo=2, m=8, c=d_codes, c2=d_codes2, shift=0, shift2=0, n_pos=codes.size, o=d_off, ln=d_len, n_rec=3, out=d_occ):
        return L.pfmscan_occupancy_pair_dev(h, p(R), p(S), n_mo, m, ptr(c, shift), ptr(c2, shift2), n_pos, ptr(o), ptr(ln), n_rec, ptr(out), None)
    assert dev(m=0) == _lib.E_BADSHAPE and dev(R=wide, S=wide, m=65) == _lib.E_BADSHAPE
    assert dev(shift=4) == _lib.E_BADSHAPE and dev(shift2=8) == _lib.E_BADSHAPE
    assert dev(R=None) == _lib.E_BADARG and dev(S=None) == _lib.E_BADARG and dev(c=None) == _lib.E_BADARG and dev(c2=None) == _lib.E_BADARG
    assert dev(o=None) == _lib.E_BADARG and dev(ln=None) == _lib.E_BADARG and dev(out=None) == _lib.E_BADARG
    assert dev(n_pos=codes.size - 2) == _lib.E_BADARG                     # the last record runs past n_pos
    swapped = torch.from_numpy(off[[1, 0, 2]].copy()).cuda()
    overlap = torch.from_numpy(np.asarray([0, 40, 112], dtype=np.int64)).cuda()
    torch.cuda.synchronize()
    assert dev(o=swapped) == _lib.E_BADARG and dev(o=overlap) == _lib.E_BADARG
    assert dev(n_mo=0) == 0 and dev(n_rec=0) == 0                         # nothing to do: OK, nothing written
    ctx.synchronize()
    assert (d_occ.cpu().numpy() == -7).all()
    assert dev() == 0
    ctx.synchronize()
    assert rules.same_bits(d_occ.cpu().numpy(), rules.occupancy(codes, codes2, off, lens, R, S)[0])
    # the staged form
    ctx.stage(codes)
    out = np.full((3, 2), -7.0)
    with pytest.raises(ValueError):
        ctx._check(L.pfmscan_occupancy_pair_staged(h, p(R), p(S), 2, 8, p(off), p(lens), 3, p(out), None))      # no codes2 staged
    ctx.stage_codes2(codes2)
    for args in ((R, S, 0), (wide, wide, 65), (None, S, 8), (R, None, 8)):
        with pytest.raises(ValueError):
            ctx._check(L.pfmscan_occupancy_pair_staged(h, p(args[0]), p(args[1]), 2, args[2], p(off), p(lens), 3, p(out), None))
    with pytest.raises(ValueError):
        ctx._check(L.pfmscan_occupancy_pair_staged(h, p(R), p(S), 2, 8, p(off), p(lens), 3, None, None))
    with pytest.raises(ValueError):
        ctx.occupancy_pair_staged(R, S, off[[1, 0, 2]], lens)
    with pytest.raises(ValueError):
        ctx.occupancy_pair_staged(R, S, off, lens + 1000)
    assert (out == -7).all()
