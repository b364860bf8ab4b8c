"""The expected counts of two code streams (k_exp_pair_blocks, csrc/pfmscan_expect.hip) on the GPU against the rules
(tests/pair_rules.py): every comparison is on the float64 bit patterns (NaN == NaN) plus equal Windows -- there is no
tolerance in the contract."""
import numpy as np
import pytest

import pair_rules as rules
from test_gpu_occupancy import length_ladder

pytestmark = pytest.mark.gpu

MODES = (rules.RATIO, rules.POSTERIOR)


def run(ctx, codes, codes2, off, lens, R, S, mode, **kw):
    ctx.stage(codes)
    ctx.stage_codes2(codes2)
    return ctx.expect_pair_staged(R, S, mode, off, lens, **kw)


def same(got, want):
    return (rules.same_bits(got[0], want[0]) and rules.same_bits(got[1], want[1]) and rules.same_bits(got[2], want[2]) and
            got[3].dtype == np.int64 and np.array_equal(got[3], want[3]))


def check(ctx, codes, codes2, off, lens, R, S, mode):
    got = run(ctx, codes, codes2, off, lens, R, S, mode)
    want = rules.expected(codes, codes2, off, lens, R, S, mode)
    for name, g, w in zip(("exp_seq", "exp_struct", "occ"), got, want):
        assert rules.same_bits(g, w), "%s bits differ at %s" % (name, np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])
    assert got[3].dtype == np.int64 and np.array_equal(got[3], want[3])
    return got


@pytest.mark.parametrize("m", [1, 8, 21, 64])
def test_record_lengths_and_widths(ctx, m):
    rng = np.random.default_rng(300 + m)
    lengths = length_ladder(rng, m)
    if m == 64:
        lengths = [min(x, 1025 + m - 1) for x in lengths]             # the rules stay within seconds
    codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.001, foreign_struct=0.001, case=True)
    R, S = rules.table(rng, m, 4, 0.6, 1.7), rules.table(rng, m, 7, 0.6, 1.7)
    n_win = np.maximum(lens - m + 1, 0)
    for n in (0, 1, 31, 32, 33, 1023, 1024, 1025) + (() if m == 64 else (32768, 32769)):
        assert (n_win == n).any()
    mode = rules.POSTERIOR if m != 8 else rules.RATIO
    got = check(ctx, codes, codes2, off, lens, R, S, mode)
    assert (got[0][n_win == 0] == 0).all() and (got[1][n_win == 0] == 0).all() and not np.signbit(got[0]).any() and not np.signbit(got[1]).any()
    assert (got[0][:, :, :, 4:] == 0).all() and (got[1][:, :, :, 7:] == 0).all() and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    # the occupancy's own bits
    occ, win = ctx.occupancy_pair_staged(R, S, off, lens)
    assert rules.same_bits(occ, got[2]) and np.array_equal(win, got[3])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [1, 8, 21])
def test_foreign_codes_in_either_stream(ctx, m, mode):
    rng = np.random.default_rng(11 * m + mode)
    L = 2 * m + 37
    n_each = L + 3
    codes, codes2, off, lens = rules.streams(rng, [L] * (3 * n_each) + [3 * m + 150] * 2, case=True)
    for which in range(3):                                            # 0: sequence only, 1: structure only, 2: both
        base = which * n_each
        for p in range(L):                                             # record p: one foreign code at position p (every offset of a window)
            if which in (0, 2):
                codes[off[base + p] + p] = np.uint8(rng.integers(4, 8))
            if which in (1, 2):
                codes2[off[base + p] + p] = np.uint8(7 | (8 if rng.random() < 0.3 else 0))
        r = base + L                                                   # foreign throughout in the stream(s) of this part
        if which in (0, 2):
            codes[off[r]:off[r] + L] = 7
        if which in (1, 2):
            codes2[off[r]:off[r] + L] = 7
    codes[off[-1] + 60:off[-1] + 60 + m + 3] = 7
    codes2[off[-2] + 30:off[-2] + 30 + m + 3] = 7
    R, S = rules.table(rng, m, 4), rules.table(rng, m, 7)
    got = check(ctx, codes, codes2, off, lens, R, S, mode)
    for which in range(3):
        r = which * n_each + L
        assert got[3][r] == 0 and got[2][r, 0] == 0 and not np.signbit(got[2][r, 0]) and (got[0][r] == 0).all() and (got[1][r] == 0).all()
        assert got[3][which * n_each] == L - m and got[3][which * n_each + L - 1] == L - m
    plain = codes2.copy()
    plain[plain != 7] &= 7
    assert (plain != codes2).any()
    assert same(run(ctx, codes, plain, off, lens, R, S, mode), got)


@pytest.mark.parametrize("mode", MODES)
def test_special_cells(ctx, mode):
    rng = np.random.default_rng(5 + mode)
    lens = [int(x) for x in rng.integers(1, 200, size=30)] + [1500]
    for m in (2, 8):
        codes, codes2, off, ln = rules.streams(rng, [x + m - 1 for x in lens], foreign_seq=0.005, foreign_struct=0.005)
        Rs, Ss = [], []
        for kind in ("zero_seq", "zero_struct", "inf_seq", "inf_struct", "nan_seq", "nan_struct", "zero_x_inf", "all_zero"):
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
                R[0, :4], S[m - 1, :7] = 0.0, np.inf
            if kind == "all_zero":
                S[0, :7] = 0.0                                         # every term +0.0: occ +0.0, every weight +0.0
            Rs.append(R)
            Ss.append(S)
        got = check(ctx, codes, codes2, off, ln, np.stack(Rs), np.stack(Ss), mode)
        assert (got[2][:, 7] == 0).all() and not np.signbit(got[2][:, 7]).any() and (got[0][:, 7] == 0).all() and (got[1][:, 7] == 0).all()
        assert np.isnan(got[2][-1, 6]) and np.isposinf(got[2][-1, 2])


def test_libraries_rows_and_scratch_passes(ctx, monkeypatch):
    """a library across the LDS chunk rule of the occupancy it runs first; PFMSCAN_OCC_SCRATCH_DOUBLES small enough to force
    record passes and passes over the matrix rows: no bit changes"""
    rng = np.random.default_rng(13)
    m = 12
    chunk = rules.lds_chunk(m)
    n_max = 2 * chunk + 3
    codes, codes2, off, lens = rules.streams(rng, [int(x) for x in rng.integers(1, 700, size=30)] + [9000] + [int(x) for x in rng.integers(1, 100, size=10)],
                                             foreign_seq=0.003, foreign_struct=0.003, case=True)
    Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(n_max)])
    Ss = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(n_max)])
    want = rules.expected(codes, codes2, off, lens, Rs, Ss, rules.POSTERIOR)
    for n in (chunk - 1, chunk, chunk + 1, n_max):
        got = run(ctx, codes, codes2, off, lens, Rs[:n], Ss[:n], rules.POSTERIOR)
        assert same(got, (want[0][:, :n], want[1][:, :n], want[2][:, :n], want[3]))
    for cap in ("1", "50", "3000", "100000"):
        monkeypatch.setenv("PFMSCAN_OCC_SCRATCH_DOUBLES", cap)
        assert same(run(ctx, codes, codes2, off, lens, Rs[:3], Ss[:3], rules.POSTERIOR), (want[0][:, :3], want[1][:, :3], want[2][:, :3], want[3]))
    monkeypatch.delenv("PFMSCAN_OCC_SCRATCH_DOUBLES")
    # either matrix alone: the same bits, the other not computed
    only_seq = run(ctx, codes, codes2, off, lens, Rs[:3], Ss[:3], rules.POSTERIOR, want_struct=False)
    assert only_seq[1] is None and rules.same_bits(only_seq[0], want[0][:, :3]) and rules.same_bits(only_seq[2], want[2][:, :3])
    monkeypatch.setenv("PFMSCAN_OCC_SCRATCH_DOUBLES", "50")
    only_struct = run(ctx, codes, codes2, off, lens, Rs[:3], Ss[:3], rules.POSTERIOR, want_seq=False)
    assert only_struct[0] is None and rules.same_bits(only_struct[1], want[1][:, :3]) and np.array_equal(only_struct[3], want[3])


@pytest.mark.parametrize("mode", MODES)
def test_independent_of_order_batch_and_stream_offset(ctx, mode):
    rng = np.random.default_rng(17 + mode)
    m = 12
    lengths = [int(x) for x in rng.integers(1, 1500, size=60)] + [5000]
    codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.002, foreign_struct=0.002, case=True)
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

    order = rng.permutation(len(recs))
    got = run(ctx, *packed(order), Rs, Ss, mode)
    assert same(got, tuple(x[order] for x in base))
    cut = 23
    a = run(ctx, *packed(range(cut)), Rs, Ss, mode)
    b = run(ctx, *packed(range(cut, len(recs))), Rs, Ss, mode)
    assert same(tuple(np.concatenate([x, y]) for x, y in zip(a, b)), base)
    for lead in (1, 2, 3):
        assert same(run(ctx, *packed(range(len(recs)), lead), Rs, Ss, mode), base)


@pytest.mark.parametrize("mode", MODES)
def test_identities_against_the_single_stream_entry_points(ctx, mode):
    rng = np.random.default_rng(19 + mode)
    for m in (8, 21):
        lengths = [int(x) + m - 1 for x in rng.integers(1, 1500, size=30)] + [m - 1, 4000]
        Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(3)])
        Ss = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(3)])
        one = np.stack([rules.ones(m)] * 3)
        codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.004, foreign_struct=0.0, case=True)
        got = run(ctx, codes, codes2, off, lens, Rs, one, mode)
        e, o, w = ctx.expect_staged(Rs, 4, mode, off, lens, 0)
        assert rules.same_bits(got[0], e) and rules.same_bits(got[2], o) and np.array_equal(got[3], w)
        codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.0, foreign_struct=0.004, case=True)
        got = run(ctx, codes, codes2, off, lens, one, Ss, mode)
        e, o, w = ctx.expect_staged(Ss, 7, mode, off, lens, 1)
        assert rules.same_bits(got[1], e) and rules.same_bits(got[2], o) and np.array_equal(got[3], w)


def test_engine_method(ctx):
    from rnascan_amd import pack, scanner
    rng = np.random.default_rng(23)
    e = scanner.HipEngine(0)
    try:
        lens = (5, 300, 0, 77)
        stream = pack.pack([rng.integers(0, 4, size=n).astype(np.uint8) for n in lens])
        stream.codes2 = pack.pack([rng.integers(0, 7, size=n).astype(np.uint8) for n in lens]).codes
        R, S = rules.table(rng, 6, 4), rules.table(rng, 6, 7)
        for mode in MODES:
            got = e.expect_pair(stream, R, S, mode)
            assert same(got, rules.expected(stream.codes, stream.codes2, stream.offsets, stream.lengths, R, S, mode))
    finally:
        e.close()


def test_dev_form_as_an_integrator_calls_it(ctx):
    """torch device tensors in and out on the context's stream; equal to the rules; nothing written outside the outputs"""
    import torch
    rng = np.random.default_rng(29)
    m, n_mo = 12, 3
    codes, codes2, off, lens = rules.streams(rng, [int(x) for x in rng.integers(1, 1200, size=40)], foreign_seq=0.003, foreign_struct=0.003, case=True)
    Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(n_mo)])
    Ss = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(n_mo)])
    want = rules.expected(codes, codes2, off, lens, Rs, Ss, rules.POSTERIOR)
    n_rec, guard, cells = len(off), 64, len(off) * n_mo * m * 8
    d_codes, d_codes2 = torch.from_numpy(codes).cuda(), torch.from_numpy(codes2).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    d_sq = torch.full((guard + cells + guard,), -7.0, dtype=torch.float64, device="cuda")
    d_st = torch.full((guard + cells + guard,), -7.0, dtype=torch.float64, device="cuda")
    d_occ = torch.full((guard + n_rec * n_mo + guard,), -7.0, dtype=torch.float64, device="cuda")
    d_win = torch.full((guard + n_rec + guard,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.expect_pair_dev(Rs, Ss, rules.POSTERIOR, d_codes.data_ptr(), d_codes2.data_ptr(), codes.size, d_off.data_ptr(), d_len.data_ptr(), n_rec,
                        d_sq.data_ptr() + 8 * guard, d_st.data_ptr() + 8 * guard, d_occ.data_ptr() + 8 * guard, d_win.data_ptr() + 8 * guard)
    ctx.synchronize()
    for t in (d_sq, d_st, d_occ, d_win):
        x = t.cpu().numpy()
        assert (x[:guard] == -7).all() and (x[-guard:] == -7).all()
    shape = (n_rec, n_mo, m, 8)
    assert rules.same_bits(d_sq.cpu().numpy()[guard:-guard].reshape(shape), want[0])
    assert rules.same_bits(d_st.cpu().numpy()[guard:-guard].reshape(shape), want[1])
    assert rules.same_bits(d_occ.cpu().numpy()[guard:-guard].reshape(n_rec, n_mo), want[2]) and np.array_equal(d_win.cpu().numpy()[guard:-guard], want[3])
    # one matrix only, no occupancy, no Windows, ratio mode
    want = rules.expected(codes, codes2, off, lens, Rs, Ss, rules.RATIO)
    d_st.fill_(-7.0)
    d_sq.fill_(-7.0)
    torch.cuda.synchronize()
    ctx.expect_pair_dev(Rs, Ss, rules.RATIO, d_codes.data_ptr(), d_codes2.data_ptr(), codes.size, d_off.data_ptr(), d_len.data_ptr(), n_rec,
                        None, d_st.data_ptr() + 8 * guard)
    ctx.synchronize()
    assert rules.same_bits(d_st.cpu().numpy()[guard:-guard].reshape(shape), want[1]) and (d_sq.cpu().numpy() == -7).all()


def test_bad_arguments_launch_nothing(ctx):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(31)
    codes, codes2, off, lens = rules.streams(rng, [50, 60, 70])
    d_codes, d_codes2 = torch.from_numpy(codes).cuda(), torch.from_numpy(codes2).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    d_sq = torch.full((3, 2, 8, 8), -7.0, dtype=torch.float64, device="cuda")
    d_st = torch.full((3, 2, 8, 8), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L, h, p = ctx._L, ctx._h, _lib._ptr
    R, S = np.ascontiguousarray(np.stack([rules.table(rng, 8, 4)] * 2)), np.ascontiguousarray(np.stack([rules.table(rng, 8, 7)] * 2))
    wide = np.ascontiguousarray(np.stack([rules.table(rng, 65, 7)] * 2))
    ptr = lambda t, shift=0: p(t.data_ptr() + shift) if t is not None else None

    def dev(R=R, S=S, n_mo=2, m=8, mode=1, c=d_codes, c2=d_codes2, shift=0, shift2=0, n_pos=codes.size, o=d_off, ln=d_len, n_rec=3, sq=d_sq, st=d_st):
        return L.pfmscan_expect_pair_dev(h, p(R), p(S), n_mo, m, mode, ptr(c, shift), ptr(c2, shift2), n_pos, ptr(o), ptr(ln), n_rec,
                                         ptr(sq), ptr(st), None, None)
    assert dev(m=0) == _lib.E_BADSHAPE and dev(R=wide, S=wide, m=65) == _lib.E_BADSHAPE
    assert dev(shift=4) == _lib.E_BADSHAPE and dev(shift2=8) == _lib.E_BADSHAPE
    assert dev(mode=2) == _lib.E_BADARG and dev(mode=-1) == _lib.E_BADARG
    assert dev(R=None) == _lib.E_BADARG and dev(S=None) == _lib.E_BADARG and dev(c=None) == _lib.E_BADARG and dev(c2=None) == _lib.E_BADARG
    assert dev(o=None) == _lib.E_BADARG and dev(ln=None) == _lib.E_BADARG and dev(sq=None, st=None) == _lib.E_BADARG
    assert dev(n_pos=codes.size - 2) == _lib.E_BADARG
    swapped = torch.from_numpy(off[[1, 0, 2]].copy()).cuda()
    torch.cuda.synchronize()
    assert dev(o=swapped) == _lib.E_BADARG
    assert dev(n_mo=0) == 0 and dev(n_rec=0) == 0                         # nothing to do: OK, nothing written
    ctx.synchronize()
    assert (d_sq.cpu().numpy() == -7).all() and (d_st.cpu().numpy() == -7).all()
    assert dev() == 0
    ctx.synchronize()
    want = rules.expected(codes, codes2, off, lens, R, S, rules.POSTERIOR)
    assert rules.same_bits(d_sq.cpu().numpy(), want[0]) and rules.same_bits(d_st.cpu().numpy(), want[1])
    # the staged form
    ctx.stage(codes)
    with pytest.raises(ValueError):
        ctx.expect_pair_staged(R, S, 1, off, lens)                         # no codes2 staged
    ctx.stage_codes2(codes2)
    with pytest.raises(ValueError):
        ctx.expect_pair_staged(R, S, 2, off, lens)
    with pytest.raises(ValueError):
        ctx.expect_pair_staged(R, S, 1, off, lens, want_seq=False, want_struct=False)
    with pytest.raises(ValueError):
        ctx.expect_pair_staged(wide, wide, 1, off, lens)
    with pytest.raises(ValueError):
        ctx.expect_pair_staged(R, S, 1, off[[1, 0, 2]], lens)
