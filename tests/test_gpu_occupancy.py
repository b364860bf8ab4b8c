"""The occupancy kernels (csrc/pfmscan_occupancy.hip) on the GPU against the rules (tests/occupancy_rules.py): every comparison
is on the float64 bit patterns (NaN == NaN) plus equal Windows -- there is no tolerance in the contract."""
import numpy as np
import pytest

import occupancy_rules as rules

pytestmark = pytest.mark.gpu

LDS_DOUBLES = 2048     # OCC_LDS_DOUBLES of csrc/pfmscan_occupancy.hip: table cells of one chunk of motifs, padding included


def lds_chunk(m, n_letters, n_q=1 << 20):
    """occ_chunk of csrc/pfmscan_occupancy.hip: motifs per LDS chunk"""
    def ls(nq):
        qn = 8 if nq >= 8 else 4 if nq >= 4 else 2 if nq >= 2 else 1
        x = -(-nq // qn) * qn
        return x + 2 if x % 16 == 0 else x
    c = max(1, min(n_q, LDS_DOUBLES // (m * n_letters)))
    while c > 1 and m * n_letters * ls(c) > LDS_DOUBLES:
        c -= 1
    return c


def run(ctx, codes, off, lens, tables, n_letters, which=0):
    ctx.stage(codes)
    if which:
        ctx.stage_codes2(codes)
    return ctx.occupancy_staged(tables, n_letters, off, lens, which)


def check(ctx, codes, off, lens, tables, n_letters):
    got = run(ctx, codes, off, lens, tables, n_letters)
    want = rules.occupancy(codes, off, lens, tables, n_letters)
    assert rules.same_bits(got[0], want[0]), "occupancy bits differ at %s" % np.argwhere(~((got[0] == want[0]) | (np.isnan(got[0]) & np.isnan(want[0]))))[:5]
    assert got[1].dtype == np.int64 and np.array_equal(got[1], want[1])
    return got


def length_ladder(rng, m):
    """n_win at 0 (L < m, L = m - 1), 1, 31, 32, 33, 1023, 1024, 1025, 32768 and 32769 (four levels), with many short
    records of 1-3 blocks before and between them: a wave holds several records, a record straddles waves and workgroups"""
    lengths = []
    for n_win in (None, 0, 1, 31, 32, 33, 1023, 1024, 1025, 32768, 32769):
        lengths += [int(x) + m - 1 for x in rng.integers(1, 97, size=int(rng.integers(20, 60)))]
        lengths.append(max(m - 3, 0) if n_win is None else n_win + m - 1)
    return lengths + [int(x) + m - 1 for x in rng.integers(1, 97, size=300)]


@pytest.fixture(scope="module")
def ladder():
    """the length ladder once per width: (codes, off, lens, table, the rules' answer)"""
    cache = {}

    def get(m):
        if m not in cache:
            rng = np.random.default_rng(100 + m)
            codes, off, lens = rules.stream(rng, length_ladder(rng, m), 4, foreign=0.002)
            R = rules.table(rng, m, 4, 0.5, 2.0)
            cache[m] = (codes, off, lens, R, rules.occupancy(codes, off, lens, R, 4))
        return cache[m]
    return get


@pytest.mark.parametrize("m", [1, 2, 8, 12, 20, 21, 64])
def test_record_lengths_and_widths(ctx, ladder, m):
    codes, off, lens, R, want = ladder(m)
    got = run(ctx, codes, off, lens, R, 4)
    assert rules.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
    n_win = np.maximum(lens - m + 1, 0)
    for n in (0, 1, 31, 32, 33, 1023, 1024, 1025, 32768, 32769):
        assert (n_win == n).any()
    assert (got[0][n_win == 0] == 0).all() and not np.signbit(got[0][n_win == 0]).any() and (got[1][n_win == 0] == 0).all()
    assert np.isfinite(got[0]).all() and (got[0][got[1] > 0] > 0).all()         # a window with a term adds a positive ratio


@pytest.mark.parametrize("n_letters", [4, 7])
@pytest.mark.parametrize("m", [1, 8, 21, 64])
def test_foreign_codes(ctx, n_letters, m):
    """a foreign code at the start, at the end, at every offset of a window, two within m of each other; on the structure
    side a third of the letters carry bit 3 and count as their letter"""
    rng = np.random.default_rng(7 * m + n_letters)
    L = 2 * m + 37
    codes, off, lens = rules.stream(rng, [L] * (L + 2 * m + 2) + [5 * m + 200] * 3, n_letters, case=n_letters == 7)
    bad = lambda: np.uint8(rng.integers(n_letters, 8))
    for p in range(L):                                               # record p: one foreign code at position p
        codes[off[p] + p] = bad()
    for d in range(1, 2 * m + 1):                                    # two of them d apart (within m and beyond)
        r = L + d
        codes[off[r] + 10], codes[off[r] + min(10 + d, L - 1)] = bad(), bad()
    r = L + 2 * m + 1
    codes[off[r]:off[r] + L] = 7                                     # nothing but foreign codes
    codes[off[-1] + 100:off[-1] + 100 + m + 3] = 7
    R = rules.table(rng, m, n_letters)
    got = check(ctx, codes, off, lens, R, n_letters)
    assert got[1][r] == 0 and got[0][r, 0] == 0
    assert got[1][0] == L - m + 1 - 1 and got[1][L - 1] == L - m + 1 - 1        # the first and the last position lie in one window each
    if n_letters == 7:
        plain = codes.copy()
        plain[plain != 7] &= 7
        assert (plain != codes).any()
        again = run(ctx, plain, off, lens, R, 7)
        assert rules.same_bits(again[0], got[0]) and np.array_equal(again[1], got[1])


@pytest.mark.parametrize("n_letters", [4, 7])
def test_special_cells(ctx, n_letters):
    """+0.0, +inf, both in one window (NaN), a NaN cell; products of 64 small ratios that go subnormal and then to 0,
    large ones that overflow"""
    rng = np.random.default_rng(n_letters)
    lens = [int(x) for x in rng.integers(1, 400, size=60)] + [3000]
    for m in (2, 8, 64):
        codes, off, ln = rules.stream(rng, [x + m - 1 for x in lens], n_letters, foreign=0.01)
        tables = []
        for kind in ("zero", "inf", "both", "nan"):
            R = rules.table(rng, m, n_letters)
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
        got = check(ctx, codes, off, ln, np.stack(tables), n_letters)[0]
        assert np.isnan(got[-1, 2]) and np.isnan(got[-1, 3]) and np.isposinf(got[-1, 1])
        if m == 64:
            t, _ = rules.terms(codes, off[-1], ln[-1], small, n_letters)
            assert ((t > 0) & (t < 2.3e-308)).any() and (t == 0).any()          # subnormal products, and products that reached 0
            assert got[-1, 4] > 0
            assert np.isposinf(got[:, 5]).any()


def test_libraries_and_chunks(ctx):
    """n_motifs at 1, 2, 3, 5, 9, one less than a full LDS chunk, a full chunk, one more, and 300: motif k's column is the
    single-motif call on table k"""
    rng = np.random.default_rng(11)
    m, n_letters = 8, 4
    full = lds_chunk(m, n_letters)
    assert 32 < full <= LDS_DOUBLES // (m * n_letters)
    codes, off, lens = rules.stream(rng, [int(x) for x in rng.integers(1, 300, size=40)] + [2500], n_letters, foreign=0.01)
    tables = np.stack([rules.table(rng, m, n_letters) for _ in range(300)])
    want = rules.occupancy(codes, off, lens, tables, n_letters)
    ctx.stage(codes)
    single = {}
    for n in (1, 2, 3, 5, 9, full - 1, full, full + 1, 300):
        occ, win = ctx.occupancy_staged(tables[:n], n_letters, off, lens)
        assert rules.same_bits(occ, want[0][:, :n]) and np.array_equal(win, want[1])
        for k in (0, n // 2, n - 1):
            if k not in single:
                single[k] = ctx.occupancy_staged(tables[k], n_letters, off, lens)[0][:, 0]
            assert rules.same_bits(occ[:, k], single[k])
    # the structure side at a width where a chunk holds few motifs
    m7 = 21
    full7 = lds_chunk(m7, 7)
    codes, off, lens = rules.stream(rng, [int(x) for x in rng.integers(1, 300, size=30)], 7, foreign=0.01, case=True)
    tables = np.stack([rules.table(rng, m7, 7) for _ in range(2 * full7 + 1)])
    for n in (full7 - 1, full7, full7 + 1, 2 * full7 + 1):
        check(ctx, codes, off, lens, tables[:n], 7)


def test_scratch_passes_change_no_bit(ctx, monkeypatch):
    """the partial sums go through bounded scratch: with a bound of a few cells the records, and for the long record the
    motifs, run in passes -- the same bits"""
    rng = np.random.default_rng(13)
    m = 12
    codes, off, lens = rules.stream(rng, [int(x) for x in rng.integers(1, 1500, size=50)] + [40000] + [int(x) for x in rng.integers(1, 200, size=20)], 4, foreign=0.005)
    tables = np.stack([rules.table(rng, m, 4, 0.5, 2.0) for _ in range(7)])
    want = check(ctx, codes, off, lens, tables, 4)
    for cap in ("1", "50", "3000", "100000"):
        monkeypatch.setenv("PFMSCAN_OCC_SCRATCH_DOUBLES", cap)
        got = run(ctx, codes, off, lens, tables, 4)
        assert rules.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_independent_of_order_batch_and_stream(ctx):
    """the same records in another order, split over two streams, and staged as codes2: the same per-record values"""
    rng = np.random.default_rng(17)
    m = 12
    lengths = [int(x) for x in rng.integers(1, 4000, size=80)] + [33000]
    codes, off, lens = rules.stream(rng, lengths, 4, foreign=0.003)
    tables = np.stack([rules.table(rng, m, 4, 0.5, 2.0) for _ in range(3)])
    base = check(ctx, codes, off, lens, tables, 4)
    recs = [codes[o:o + n] for o, n in zip(off, lens)]

    def packed(order):
        ln = np.asarray([recs[i].size for i in order], dtype=np.int64)
        of = np.zeros(ln.size, dtype=np.int64)
        of[1:] = np.cumsum(ln[:-1] + 1)
        c = np.full(int((ln + 1).sum()), 7, dtype=np.uint8)
        for o, i in zip(of, order):
            c[o:o + recs[i].size] = recs[i]
        return c, of, ln

    order = rng.permutation(len(recs))
    got = run(ctx, *packed(order), tables, 4)
    assert rules.same_bits(got[0], base[0][order]) and np.array_equal(got[1], base[1][order])
    cut = 37
    a = run(ctx, *packed(range(cut)), tables, 4)
    b = run(ctx, *packed(range(cut, len(recs))), tables, 4)
    assert rules.same_bits(np.concatenate([a[0], b[0]]), base[0]) and np.array_equal(np.concatenate([a[1], b[1]]), base[1])
    # a record table that names only some records of the staged stream, in place
    some = np.sort(rng.choice(len(recs), size=20, replace=False))
    ctx.stage(codes)
    part = ctx.occupancy_staged(tables, 4, off[some], lens[some])
    assert rules.same_bits(part[0], base[0][some]) and np.array_equal(part[1], base[1][some])
    # which = 1: the same bytes as codes2, under other codes
    ctx.stage(np.full(codes.size, 7, dtype=np.uint8))
    ctx.stage_codes2(codes)
    second = ctx.occupancy_staged(tables, 4, off, lens, which=1)
    assert rules.same_bits(second[0], base[0]) and np.array_equal(second[1], base[1])
    first = ctx.occupancy_staged(tables, 4, off, lens, which=0)
    assert (first[0] == 0).all() and (first[1] == 0).all()


def test_engine_method(ctx):
    from rnascan_amd import pack, scanner
    rng = np.random.default_rng(19)
    e = scanner.HipEngine(0)
    try:
        recs = [rng.integers(0, 4, size=int(n)).astype(np.uint8) for n in (5, 300, 0, 77)]
        stream = pack.pack(recs)
        R = rules.table(rng, 6, 4)
        occ, win = e.occupancy(stream, R, 4)
        want = rules.occupancy(stream.codes, stream.offsets, stream.lengths, R, 4)
        assert rules.same_bits(occ, want[0]) and np.array_equal(win, want[1])
        stream.codes2 = stream.codes
        occ2, win2 = e.occupancy(stream, R[None], 4, which=1)
        assert rules.same_bits(occ2, occ) and np.array_equal(win2, win)
    finally:
        e.close()


def test_dev_form_as_an_integrator_calls_it(ctx):
    """torch device tensors in and out; equal to _staged; nothing written outside [n_rec][n_motifs] and [n_rec]"""
    import torch
    rng = np.random.default_rng(23)
    m, n_mo = 12, 5
    codes, off, lens = rules.stream(rng, [int(x) for x in rng.integers(1, 2000, size=60)], 4, foreign=0.004)
    tables = np.stack([rules.table(rng, m, 4, 0.5, 2.0) for _ in range(n_mo)])
    want = run(ctx, codes, off, lens, tables, 4)
    n_rec, guard = len(off), 64
    d_codes, d_off, d_len = torch.from_numpy(codes).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    d_occ = torch.full((guard + n_rec * n_mo + guard,), -7.0, dtype=torch.float64, device="cuda")
    d_win = torch.full((guard + n_rec + guard,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.occupancy_dev(tables, 4, d_codes.data_ptr(), codes.size, d_off.data_ptr(), d_len.data_ptr(), n_rec,
                      d_occ.data_ptr() + 8 * guard, d_win.data_ptr() + 8 * guard)
    ctx.synchronize()
    occ, win = d_occ.cpu().numpy(), d_win.cpu().numpy()
    assert (occ[:guard] == -7).all() and (occ[-guard:] == -7).all() and (win[:guard] == -7).all() and (win[-guard:] == -7).all()
    assert rules.same_bits(occ[guard:-guard].reshape(n_rec, n_mo), want[0]) and np.array_equal(win[guard:-guard], want[1])
    # without Windows
    d_occ.fill_(-7.0)
    torch.cuda.synchronize()
    ctx.occupancy_dev(tables, 4, d_codes.data_ptr(), codes.size, d_off.data_ptr(), d_len.data_ptr(), n_rec, d_occ.data_ptr() + 8 * guard, None)
    ctx.synchronize()
    assert rules.same_bits(d_occ.cpu().numpy()[guard:-guard].reshape(n_rec, n_mo), want[0])


def test_bad_arguments_launch_nothing(ctx):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(29)
    codes, off, lens = rules.stream(rng, [50, 60, 70], 4)
    d_codes, d_off, d_len = torch.from_numpy(codes).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    d_occ = torch.full((3, 2), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L, h = ctx._L, ctx._h
    R = np.ascontiguousarray(np.stack([rules.table(rng, 8, 4)] * 2))
    wide = np.ascontiguousarray(np.stack([rules.table(rng, 65, 4)] * 2))
    p = _lib._ptr

    def dev(tables, n_mo, m, nl, c=d_codes, n_pos=codes.size, o=d_off, ln=d_len, n_rec=3, out=d_occ):
        return L.pfmscan_occupancy_dev(h, p(tables), n_mo, m, nl, p(c.data_ptr()) if c is not None else None, n_pos,
                                       p(o.data_ptr()) if o is not None else None, p(ln.data_ptr()) if ln is not None else None, n_rec,
                                       p(out.data_ptr()) if out is not None else None, None)
    assert dev(R, 2, 0, 4) == _lib.E_BADSHAPE and dev(wide, 2, 65, 4) == _lib.E_BADSHAPE
    assert dev(R, 2, 8, 5) == _lib.E_BADARG and dev(R, 2, 8, 8) == _lib.E_BADARG
    assert dev(None, 2, 8, 4) == _lib.E_BADARG and dev(R, 2, 8, 4, c=None) == _lib.E_BADARG
    assert dev(R, 2, 8, 4, o=None) == _lib.E_BADARG and dev(R, 2, 8, 4, ln=None) == _lib.E_BADARG and dev(R, 2, 8, 4, out=None) == _lib.E_BADARG
    assert dev(R, 2, 8, 4, n_pos=codes.size - 2) == _lib.E_BADARG                 # the last record runs past n_pos (its separator is the last byte)
    swapped = torch.from_numpy(off[[1, 0, 2]].copy()).cuda()
    overlap = torch.from_numpy(np.asarray([0, 40, 112], dtype=np.int64)).cuda()
    torch.cuda.synchronize()
    assert dev(R, 2, 8, 4, o=swapped) == _lib.E_BADARG and dev(R, 2, 8, 4, o=overlap) == _lib.E_BADARG
    assert dev(R, 0, 8, 4) == 0 and dev(R, 2, 8, 4, n_rec=0) == 0                  # nothing to do: OK, nothing written
    ctx.synchronize()
    assert (d_occ.cpu().numpy() == -7).all()
    assert dev(R, 2, 8, 4) == 0
    ctx.synchronize()
    assert rules.same_bits(d_occ.cpu().numpy(), rules.occupancy(codes, off, lens, R, 4)[0])
    # the staged form: the same codes
    ctx.stage(codes)
    for args in ((0, R, 0, 4), (0, wide, 65, 4), (0, R, 8, 5), (2, R, 8, 4)):
        with pytest.raises(ValueError):
            out = np.zeros((3, 2))
            ctx._check(L.pfmscan_occupancy_staged(h, args[0], p(args[1]), 2, args[2], args[3], p(off), p(lens), 3, p(out), None))
    with pytest.raises(ValueError):
        ctx.occupancy_staged(R, 4, off[[1, 0, 2]], lens)
    with pytest.raises(ValueError):
        ctx.occupancy_staged(R, 4, off, lens + 1000)
    ctx.stage(codes)
    with pytest.raises(ValueError):
        ctx.occupancy_staged(R, 4, off, lens, which=1)                              # no codes2 staged
