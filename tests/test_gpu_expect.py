"""The expected-counts kernels (csrc/pfmscan_expect.hip) on the GPU against the rules (tests/expect_rules.py): every comparison
is on the float64 bit patterns (NaN == NaN) plus equal Windows -- there is no tolerance in the contract."""
import numpy as np
import pytest

import expect_rules as rules
import occupancy_rules as orules
from test_gpu_occupancy import length_ladder

pytestmark = pytest.mark.gpu

MODES = (rules.RATIO, rules.POSTERIOR)


def run(ctx, codes, off, lens, tables, n_letters, mode, which=0):
    if which:
        ctx.stage(np.full(codes.size, 7, dtype=np.uint8))           # the codes are read from codes2 and from nowhere else
        ctx.stage_codes2(codes)
    else:
        ctx.stage(codes)
    return ctx.expect_staged(tables, n_letters, mode, off, lens, which)


def same(got, want):
    return (rules.same_bits(got[0], want[0]) and rules.same_bits(got[1], want[1]) and got[2].dtype == np.int64 and np.array_equal(got[2], want[2]))


def check(ctx, codes, off, lens, tables, n_letters, mode, which=0):
    got = run(ctx, codes, off, lens, tables, n_letters, mode, which)
    want = rules.expected(codes, off, lens, tables, n_letters, mode)
    assert rules.same_bits(got[1], want[1]) and np.array_equal(got[2], want[2])
    bad = np.argwhere(~((got[0] == want[0]) | (np.isnan(got[0]) & np.isnan(want[0]))))
    assert rules.same_bits(got[0], want[0]), "expected-count bits differ at (record, motif, k, c) %s" % bad[:5]
    return got


def short_ladder(rng, m):
    """n_win 0 .. 1025 with short records between: a wave holds several records, a record straddles workgroups"""
    lengths = []
    for n_win in (None, 0, 1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025):
        lengths += [int(x) + m - 1 for x in rng.integers(1, 97, size=int(rng.integers(5, 15)))]
        lengths.append(max(m - 3, 0) if n_win is None else n_win + m - 1)
    return lengths + [int(x) + m - 1 for x in rng.integers(1, 97, size=40)]


@pytest.fixture(scope="module")
def ladder():
    """the length ladder once per width: the stream and table, and the rules' answer once per mode"""
    streams, answers = {}, {}

    def get(m, mode):
        if m not in streams:
            rng = np.random.default_rng(200 + m)
            codes, off, lens = orules.stream(rng, length_ladder(rng, m), 4, foreign=0.002)
            streams[m] = (codes, off, lens, orules.table(rng, m, 4, 0.5, 2.0))
        if (m, mode) not in answers:
            codes, off, lens, R = streams[m]
            answers[(m, mode)] = rules.expected(codes, off, lens, R, 4, mode)
        return streams[m] + (answers[(m, mode)],)
    return get


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [1, 2, 8, 12, 20, 21, 64])
def test_record_lengths_and_widths(ctx, ladder, m, mode):
    codes, off, lens, R, want = ladder(m, mode)
    got = run(ctx, codes, off, lens, R, 4, mode)
    assert same(got, want)
    n_win = np.maximum(lens - m + 1, 0)
    for n in (0, 1, 31, 32, 33, 1023, 1024, 1025, 32768, 32769):
        assert (n_win == n).any()
    assert (got[0][n_win == 0] == 0).all() and not np.signbit(got[0]).any() and np.isfinite(got[0]).all()
    assert (got[0][:, :, :, 4:] == 0).all()
    if m == 12:                                                       # d_occ and Windows are the occupancy's own
        ctx.stage(codes)
        occ, win = ctx.occupancy_staged(R, 4, off, lens)
        assert rules.same_bits(got[1], occ) and np.array_equal(got[2], win)


@pytest.mark.parametrize("m", [7, 9, 15, 16, 17, 31, 32, 33, 34, 63])
def test_widths_around_the_kernel_s_boundaries(ctx, m):
    """a lane adds one cell per round of 32 cells (4 m cells: rounds change at m = 8, 16), and parks one code per round of 32
    codes (32 + m - 1 codes: rounds change at m = 1, 33)"""
    rng = np.random.default_rng(300 + m)
    codes, off, lens = orules.stream(rng, short_ladder(rng, m), 4, foreign=0.003)
    R = orules.table(rng, m, 4, 0.5, 2.0)
    for mode in MODES:
        check(ctx, codes, off, lens, R, 4, mode)


@pytest.mark.parametrize("m", [1, 4, 5, 9, 10, 21, 64])
def test_structure_letters_from_codes2(ctx, m):
    """n_letters = 7 over codes2 (7 m cells: rounds of 32 change at m = 4 / 5, 9 / 10); a third of the letters carry bit 3"""
    rng = np.random.default_rng(400 + m)
    codes, off, lens = orules.stream(rng, short_ladder(rng, m), 7, foreign=0.003, case=True)
    R = orules.table(rng, m, 7, 0.5, 2.0)
    for mode in MODES:
        got = check(ctx, codes, off, lens, R, 7, mode, which=1)
        assert (got[0][:, :, :, 7:] == 0).all()
    plain = codes.copy()
    plain[plain != 7] &= 7
    assert (plain != codes).any()
    assert same(run(ctx, plain, off, lens, R, 7, rules.POSTERIOR, which=1), got)


@pytest.mark.parametrize("n_letters", [4, 7])
@pytest.mark.parametrize("m", [1, 8, 21, 64])
def test_foreign_codes(ctx, n_letters, m):
    """a foreign code at the start, at the end, at every offset of a window, two within m of each other, a record of
    nothing else"""
    rng = np.random.default_rng(7 * m + n_letters)
    L = 2 * m + 37
    codes, off, lens = orules.stream(rng, [L] * (L + 2 * m + 2) + [5 * m + 200] * 3, n_letters, case=n_letters == 7)
    bad = lambda: np.uint8(rng.integers(n_letters, 8))
    for p in range(L):                                               # record p: one foreign code at position p
        codes[off[p] + p] = bad()
    for d in range(1, 2 * m + 1):                                    # two of them d apart (within m and beyond)
        r = L + d
        codes[off[r] + 10], codes[off[r] + min(10 + d, L - 1)] = bad(), bad()
    r = L + 2 * m + 1
    codes[off[r]:off[r] + L] = 7                                     # nothing but foreign codes
    codes[off[-1] + 100:off[-1] + 100 + m + 3] = 7
    R = orules.table(rng, m, n_letters)
    for mode in MODES:
        got = check(ctx, codes, off, lens, R, n_letters, mode, which=int(n_letters == 7))
        assert got[2][r] == 0 and got[1][r, 0] == 0 and (got[0][r] == 0).all() and not np.signbit(got[0][r]).any()


@pytest.mark.parametrize("n_letters", [4, 7])
def test_special_cells_and_several_motifs(ctx, n_letters):
    """+0.0, +inf, both in one window (NaN), a NaN cell; products of 64 small ratios that go subnormal and then to 0, large
    ones that overflow -- six motifs of one width in one call"""
    rng = np.random.default_rng(n_letters)
    lens = [int(x) for x in rng.integers(1, 300, size=30)] + [1500]
    for m in (2, 8, 64):
        codes, off, ln = orules.stream(rng, [x + m - 1 for x in lens], n_letters, foreign=0.01)
        tables = []
        for kind in ("zero", "inf", "both", "nan"):
            R = orules.table(rng, m, n_letters)
            if kind in ("zero", "both"):
                R[0, 1] = 0.0
            if kind in ("inf", "both"):
                R[m - 1, 2] = np.inf
            if kind == "nan":
                R[m // 2, 0] = np.nan
            tables.append(R)
        small = np.full((m, 8), np.nan)
        small[:, :n_letters] = rng.choice([1e-5, 1e-6, 2e-5, 3e-5], size=(m, n_letters))
        large = np.full((m, 8), np.nan)
        large[:, :n_letters] = rng.choice([1e4, 1e5, 1e6, 7e4], size=(m, n_letters))
        tables += [small, large]
        tables = np.stack(tables)
        for mode in MODES:
            got = check(ctx, codes, off, ln, tables, n_letters, mode, which=int(n_letters == 7))
            assert np.isnan(got[0][-1, 2]).any() and np.isnan(got[0][-1, 3]).any()
            if mode == rules.RATIO:
                assert np.isposinf(got[0][-1, 1]).any()
                if m == 64:
                    x = got[0][:, 4]
                    assert ((x > 0) & (x < 2.3e-308)).any()              # subnormal sums of subnormal products stay
            for k in range(tables.shape[0]):                             # motif k's matrices are the single-motif call on table k
                if k in (0, 5):
                    one = ctx.expect_staged(tables[k], n_letters, mode, off, ln, int(n_letters == 7))
                    assert rules.same_bits(one[0][:, 0], got[0][:, k]) and rules.same_bits(one[1][:, 0], got[1][:, k])


def test_zero_occupancy_in_posterior_mode(ctx):
    """a record whose occupancy is +0.0 (every term 0, or no window with a term) gives +0.0 in every cell, not -0.0 or NaN"""
    rng = np.random.default_rng(31)
    m = 6
    codes, off, lens = orules.stream(rng, [40, 200, 3, 90, 1200], 4)
    codes[off[1]:off[1] + 200] = 2                                    # record 1: only letter 2, whose first ratio is 0
    codes[off[3]:off[3] + 90:4] = 7                                   # record 3: a foreign code in every window
    R = orules.table(rng, m, 4)
    R[0, 2] = 0.0
    got = check(ctx, codes, off, lens, R, 4, rules.POSTERIOR)
    for r in (1, 2, 3):
        assert got[1][r, 0] == 0 and (got[0][r].view(np.uint64) == 0).all()
    assert got[2].tolist()[1:4] == [195, 0, 0] and got[1][0, 0] > 0


def test_scratch_passes_change_no_bit(ctx, monkeypatch):
    """with a bound of a few cells the records, and for the long record the cells and motifs, run in passes"""
    rng = np.random.default_rng(13)
    m = 8
    codes, off, lens = orules.stream(rng, [int(x) for x in rng.integers(1, 700, size=25)] + [5000] + [int(x) for x in rng.integers(1, 200, size=8)], 4,
                                     foreign=0.005)
    tables = np.stack([orules.table(rng, m, 4, 0.5, 2.0) for _ in range(3)])
    for mode in MODES:
        want = check(ctx, codes, off, lens, tables, 4, mode)
        for cap in ("1", "3000", "7000", "100000"):                   # 157 blocks in the long record: 1, 19, 44 and all 96 columns per pass
            monkeypatch.setenv("PFMSCAN_OCC_SCRATCH_DOUBLES", cap)
            assert same(run(ctx, codes, off, lens, tables, 4, mode), want)
        monkeypatch.delenv("PFMSCAN_OCC_SCRATCH_DOUBLES")


def test_independent_of_order_batch_and_stream(ctx):
    """the same records in another order, split over two streams, behind a subset record table: the same per-record bits"""
    rng = np.random.default_rng(17)
    m = 12
    lengths = [int(x) for x in rng.integers(1, 2000, size=60)] + [33000]
    codes, off, lens = orules.stream(rng, lengths, 4, foreign=0.003)
    tables = np.stack([orules.table(rng, m, 4, 0.5, 2.0) for _ in range(2)])
    recs = [codes[o:o + n] for o, n in zip(off, lens)]

    def packed(order):
        ln = np.asarray([recs[i].size for i in order], dtype=np.int64)
        of = np.zeros(ln.size, dtype=np.int64)
        of[1:] = np.cumsum(ln[:-1] + 1)
        c = np.full(int((ln + 1).sum()), 7, dtype=np.uint8)
        for o, i in zip(of, order):
            c[o:o + recs[i].size] = recs[i]
        return c, of, ln

    for mode in MODES:
        base = check(ctx, codes, off, lens, tables, 4, mode)
        order = rng.permutation(len(recs))
        assert same(run(ctx, *packed(order), tables, 4, mode), tuple(x[order] for x in base))
        cut = 37
        a = run(ctx, *packed(range(cut)), tables, 4, mode)
        b = run(ctx, *packed(range(cut, len(recs))), tables, 4, mode)
        assert same(tuple(np.concatenate([x, y]) for x, y in zip(a, b)), base)
        some = np.sort(rng.choice(len(recs), size=20, replace=False))
        ctx.stage(codes)
        assert same(ctx.expect_staged(tables, 4, mode, off[some], lens[some]), tuple(x[some] for x in base))


def test_engine_method(ctx):
    from rnascan_amd import _lib, pack, scanner
    rng = np.random.default_rng(19)
    e = scanner.HipEngine(0)
    try:
        recs = [rng.integers(0, 4, size=int(n)).astype(np.uint8) for n in (5, 300, 0, 77)]
        stream = pack.pack(recs)
        R = orules.table(rng, 6, 4)
        for mode, name in ((rules.RATIO, _lib.EXPECT_RATIO), (rules.POSTERIOR, _lib.EXPECT_POSTERIOR)):
            got = e.expect(stream, R, 4, name)
            assert same(got, rules.expected(stream.codes, stream.offsets, stream.lengths, R, 4, mode))
            stream.codes2 = stream.codes
            assert same(e.expect(stream, R[None], 4, name, which=1), got)
    finally:
        e.close()


def test_dev_form_as_an_integrator_calls_it(ctx):
    """torch device tensors in and out; equal to _staged; nothing written outside the outputs; occ and windows optional"""
    import torch
    rng = np.random.default_rng(23)
    m, n_mo = 12, 3
    codes, off, lens = orules.stream(rng, [int(x) for x in rng.integers(1, 2000, size=40)], 4, foreign=0.004)
    tables = np.stack([orules.table(rng, m, 4, 0.5, 2.0) for _ in range(n_mo)])
    n_rec, guard = len(off), 64
    d_codes, d_off, d_len = torch.from_numpy(codes).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    for mode in MODES:
        want = run(ctx, codes, off, lens, tables, 4, mode)
        d_exp = torch.full((guard + n_rec * n_mo * m * 8 + guard,), -7.0, dtype=torch.float64, device="cuda")
        d_occ = torch.full((guard + n_rec * n_mo + guard,), -7.0, dtype=torch.float64, device="cuda")
        d_win = torch.full((guard + n_rec + guard,), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.expect_dev(tables, 4, mode, d_codes.data_ptr(), codes.size, d_off.data_ptr(), d_len.data_ptr(), n_rec,
                       d_exp.data_ptr() + 8 * guard, d_occ.data_ptr() + 8 * guard, d_win.data_ptr() + 8 * guard)
        ctx.synchronize()
        exp, occ, win = d_exp.cpu().numpy(), d_occ.cpu().numpy(), d_win.cpu().numpy()
        for x in (exp, occ, win):
            assert (x[:guard] == -7).all() and (x[-guard:] == -7).all()
        assert same((exp[guard:-guard].reshape(n_rec, n_mo, m, 8), occ[guard:-guard].reshape(n_rec, n_mo), win[guard:-guard]), want)
        d_exp.fill_(-7.0)                                             # without the occupancy and Windows
        torch.cuda.synchronize()
        ctx.expect_dev(tables, 4, mode, d_codes.data_ptr(), codes.size, d_off.data_ptr(), d_len.data_ptr(), n_rec, d_exp.data_ptr() + 8 * guard)
        ctx.synchronize()
        assert rules.same_bits(d_exp.cpu().numpy()[guard:-guard].reshape(n_rec, n_mo, m, 8), want[0])


def test_bad_record_table_launches_nothing(ctx):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(29)
    codes, off, lens = orules.stream(rng, [50, 60, 70], 4)
    d_codes, d_off, d_len = torch.from_numpy(codes).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    d_exp = torch.full((3, 2, 8, 8), -7.0, dtype=torch.float64, device="cuda")
    d_occ = torch.full((3, 2), -7.0, dtype=torch.float64, device="cuda")
    d_win = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L, h = ctx._L, ctx._h
    R = np.ascontiguousarray(np.stack([orules.table(rng, 8, 4)] * 2))
    wide = np.ascontiguousarray(np.stack([orules.table(rng, 65, 4)] * 2))
    p = _lib._ptr

    def dev(tables, n_mo, m, nl, mode=1, n_pos=codes.size, o=d_off, ln=d_len, n_rec=3, out=d_exp):
        return L.pfmscan_expect_dev(h, p(tables), n_mo, m, nl, mode, p(d_codes.data_ptr()), n_pos, p(o.data_ptr()), p(ln.data_ptr()), n_rec,
                                    p(out.data_ptr()) if out is not None else None, p(d_occ.data_ptr()), p(d_win.data_ptr()))
    swapped = torch.from_numpy(off[[1, 0, 2]].copy()).cuda()
    overlap = torch.from_numpy(np.asarray([0, 40, 112], dtype=np.int64)).cuda()
    longer = torch.from_numpy(lens + 1000).cuda()
    torch.cuda.synchronize()
    assert dev(R, 2, 8, 4, o=swapped) == _lib.E_BADARG and dev(R, 2, 8, 4, o=overlap) == _lib.E_BADARG
    assert dev(R, 2, 8, 4, ln=longer) == _lib.E_BADARG                             # the records leave the stream
    assert dev(R, 2, 8, 4, n_pos=codes.size - 2) == _lib.E_BADARG                 # the last record runs past n_pos
    assert dev(R, 2, 0, 4) == _lib.E_BADSHAPE and dev(wide, 2, 65, 4) == _lib.E_BADSHAPE
    assert dev(R, 2, 8, 5) == _lib.E_BADARG and dev(R, 2, 8, 4, mode=2) == _lib.E_BADARG and dev(R, 2, 8, 4, out=None) == _lib.E_BADARG
    assert dev(R, 0, 8, 4) == 0 and dev(R, 2, 8, 4, n_rec=0) == 0                  # nothing to do: OK, nothing written
    ctx.synchronize()
    assert (d_exp.cpu().numpy() == -7).all() and (d_occ.cpu().numpy() == -7).all() and (d_win.cpu().numpy() == -7).all()
    assert dev(R, 2, 8, 4) == 0
    ctx.synchronize()
    want = rules.expected(codes, off, lens, R, 4, rules.POSTERIOR)
    assert same((d_exp.cpu().numpy(), d_occ.cpu().numpy(), d_win.cpu().numpy()), want)
    ctx.stage(codes)
    with pytest.raises(ValueError):
        ctx.expect_staged(R, 4, rules.POSTERIOR, off[[1, 0, 2]], lens)
    with pytest.raises(ValueError):
        ctx.expect_staged(R, 4, rules.POSTERIOR, off, lens + 1000)
    with pytest.raises(ValueError):
        ctx.expect_staged(R, 4, rules.POSTERIOR, off, lens, which=1)                # no codes2 staged
