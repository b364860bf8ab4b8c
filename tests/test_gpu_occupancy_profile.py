"""k_occ_profile_blocks (csrc/pfmscan_occupancy.hip) on the GPU against the rules (tests/occupancy_profile_rules.py): every
comparison is on the float64 bit patterns (NaN == NaN) plus equal Windows -- there is no tolerance in the contract.  The
separator rows of every stream hold NaN: a kernel that read one as data would show it."""
import numpy as np
import pytest

import occupancy_profile_rules as rules
import occupancy_rules as orules

pytestmark = pytest.mark.gpu

CHUNK = 32             # OCCP_CHUNK of csrc/pfmscan_occupancy.hip: motifs a workgroup walks over the rows it staged
QN = 8                 # the most motifs whose product chains a lane advances together (then 4, 2, 1)


def run(ctx, codes, profile, off, lens, st, sq=None):
    ctx.stage(codes if sq is not None else None, profile)
    return ctx.occupancy_profile_staged(st, sq, off, lens)


def where(got, want):
    return np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5]


def check(ctx, codes, profile, off, lens, st, sq=None):
    got = run(ctx, codes, profile, off, lens, st, sq)
    want = rules.occupancy(profile, off, lens, st, codes, sq)
    assert rules.same_bits(got[0], want[0]), "occupancy bits differ at %s" % where(got[0], want[0])
    assert got[1].dtype == np.int64 and np.array_equal(got[1], want[1])
    return got


def length_ladder(rng, m):
    """n_win at 0 (L < m, L = m - 1), 1, 31-33, 255-257 (a run of 8 blocks and one window more), 1023-1025, 32768 and
    32769, among hundreds of records of 1-3 blocks: a record ends inside a workgroup's run, and a record straddles runs"""
    lengths = []
    for n_win in (None, 0, 1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 32768, 32769):
        lengths += [int(x) + m - 1 for x in rng.integers(1, 97, size=int(rng.integers(15, 40)))]
        lengths.append(max(m - 3, 0) if n_win is None else n_win + m - 1)
    return lengths + [int(x) + m - 1 for x in rng.integers(1, 97, size=200)]


LADDER_N_WIN = (0, 1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 32768, 32769)


@pytest.fixture(scope="module")
def ladder():
    """the length ladder once per (width, row dtype): the stream, one table of each kind and the rules' two answers"""
    cache = {}

    def get(m, dtype):
        if (m, dtype) not in cache:
            rng = np.random.default_rng(200 + m)
            codes, profile, off, lens = rules.stream(rng, length_ladder(rng, m), dtype, foreign=0.002)
            st, sq = rules.struct_table(rng, m, 0.5, 2.0), orules.table(rng, m, 4, 0.5, 2.0)
            cache[(m, dtype)] = (codes, profile, off, lens, st, sq, rules.occupancy(profile, off, lens, st),
                                 rules.occupancy(profile, off, lens, st, codes, sq))
        return cache[(m, dtype)]
    return get


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m", [1, 2, 8, 12, 21, 63, 64])
def test_record_lengths_widths_dtypes_and_modes(ctx, ladder, m, dtype):
    codes, profile, off, lens, st, sq, want_s, want_j = ladder(m, dtype)
    n_win = np.maximum(lens - m + 1, 0)
    for n in LADDER_N_WIN:
        assert (n_win == n).any()
    got = run(ctx, codes, profile, off, lens, st)
    assert rules.same_bits(got[0], want_s[0]), where(got[0], want_s[0])
    assert np.array_equal(got[1], n_win) and np.array_equal(got[1], want_s[1])      # structure only: every window has a term
    assert (got[0][n_win == 0] == 0).all() and not np.signbit(got[0][n_win == 0]).any()
    assert np.isfinite(got[0]).all()                                                # no separator row (NaN) was read as data
    got = run(ctx, codes, profile, off, lens, st, sq)
    assert rules.same_bits(got[0], want_j[0]), where(got[0], want_j[0])
    assert np.array_equal(got[1], want_j[1]) and (got[1] <= n_win).all() and (got[1] < n_win).any()
    assert np.isfinite(got[0]).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_base_case(ctx, dtype):
    """the case of which tests/test_occupancy_profile_cpu.py shows that a contracted marginal, float32 accumulation, the
    reversed column order and a shifted window each give other bits"""
    codes, profile, off, lens, st, sq = rules.base_case(dtype=dtype)
    check(ctx, codes, profile, off, lens, st)
    check(ctx, codes, profile, off, lens, st, sq)


@pytest.mark.parametrize("m", [1, 8, 21, 64])
def test_joint_foreign_codes(ctx, m):
    """a foreign code at every position of a record, two of them 1 .. 2 m apart, a record of nothing but foreign codes; in
    structure-only mode the same codes change nothing"""
    rng = np.random.default_rng(7 * m)
    L = 2 * m + 37
    codes, profile, off, lens = rules.stream(rng, [L] * (L + 2 * m + 2) + [5 * m + 300] * 3, np.float32)
    bad = lambda: np.uint8(rng.integers(4, 8))
    for p in range(L):
        codes[off[p] + p] = bad()
    for d in range(1, 2 * m + 1):
        r = L + d
        codes[off[r] + 10], codes[off[r] + min(10 + d, L - 1)] = bad(), bad()
    r = L + 2 * m + 1
    codes[off[r]:off[r] + L] = 7
    codes[off[-1] + 100:off[-1] + 100 + m + 3] = 7
    st, sq = rules.struct_table(rng, m), orules.table(rng, m)
    got = check(ctx, codes, profile, off, lens, st, sq)
    assert got[1][r] == 0 and got[0][r, 0] == 0
    assert got[1][0] == L - m + 1 - 1 and got[1][L - 1] == L - m + 1 - 1
    only = check(ctx, codes, profile, off, lens, st)
    assert (only[1] == np.maximum(lens - m + 1, 0)).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_cells(ctx, dtype):
    """profile rows with exact zeros (every stream has them), a NaN, a +inf and a negative cell; table cells +0.0, +inf
    (with a zero beside it in the row: 0 x inf = NaN), NaN; products that go subnormal, reach 0 and overflow"""
    rng = np.random.default_rng(31)
    lens = [int(x) for x in rng.integers(4, 400, size=60)] + [3000]                 # every record has the rows touched below
    for m in (2, 8, 64):
        codes, profile, off, ln = rules.stream(rng, [x + m - 1 for x in lens], dtype, foreign=0.01)
        assert (profile[off[0]:off[0] + ln[0]] == 0).any()
        profile[off[3] + 1, 2] = np.nan
        profile[off[5] + 2, 0] = np.inf
        profile[off[7] + 3, 4] = -0.25
        profile[off[9]:off[9] + ln[9]] = 0.0                            # a record of zero rows
        profile[off[9], 1] = -1.0                                       # ... and one negative cell: -0.0 products
        tables = []
        for kind in ("plain", "zero", "inf", "nan"):
            S = rules.struct_table(rng, m)
            if kind == "zero":
                S[0, 1] = 0.0
                S[m - 1] = 0.0
            if kind == "inf":
                S[m - 1, 2] = np.inf                                    # rows with an exact zero in column 2: NaN
            if kind == "nan":
                S[m // 2, 0] = np.nan
            tables.append(S)
        tables += [rng.choice([1e-5, 1e-6, 2e-5, 3e-5], size=(m, 7)), rng.choice([1e4, 1e5, 1e6, 7e4], size=(m, 7))]
        st = np.stack(tables)
        sq = np.stack([orules.table(rng, m) for _ in tables])
        got = check(ctx, codes, profile, off, ln, st)[0]
        check(ctx, codes, profile, off, ln, st, sq)
        assert np.isnan(got[3, 0]) and np.isnan(got[-1, 2]) and np.isnan(got[-1, 3])
        clean = np.ones(len(ln), dtype=bool)
        clean[[3, 5]] = False                                           # NaN and inf rows: 0 x inf
        assert (got[clean, 1] == 0).all()                               # a zero motif row: every term is 0
        if m == 64:
            t, _ = rules.terms(profile, off[-1], ln[-1], st[4])
            assert ((t > 0) & (t < 2.3e-308)).any() and (t == 0).any()   # subnormal products, and products that reached 0
            assert np.isposinf(got[:, 5]).any()


def test_libraries(ctx):
    """n_motifs at 1, 2, 3, 5, QN -+ 1, the workgroup's chunk -+ 1 and 300: motif k's column is the single-motif call on
    table k, in both modes"""
    rng = np.random.default_rng(11)
    m = 8
    codes, profile, off, lens = rules.stream(rng, [int(x) for x in rng.integers(1, 300, size=40)] + [2500], np.float32, foreign=0.01)
    st = np.stack([rules.struct_table(rng, m) for _ in range(300)])
    sq = np.stack([orules.table(rng, m) for _ in range(300)])
    for tabs in (None, sq):
        sub = lambda a, b=None: None if tabs is None else (tabs[a] if b is None else tabs[a:b])
        ctx.stage(codes, profile)
        full = ctx.occupancy_profile_staged(st, tabs, off, lens)
        single = dict((k, ctx.occupancy_profile_staged(st[k], sub(k), off, lens)) for k in (0, 1, 2, 4, QN, CHUNK - 1, CHUNK, 150, 299))
        for k, (occ, win) in single.items():
            want = rules.occupancy(profile, off, lens, st[k], codes, sub(k))
            assert rules.same_bits(occ, want[0]) and np.array_equal(win, want[1])
            assert rules.same_bits(full[0][:, k], occ[:, 0]) and np.array_equal(full[1], win)
        for n in (2, 3, 5, QN - 1, QN + 1, CHUNK - 1, CHUNK, CHUNK + 1):
            occ, win = ctx.occupancy_profile_staged(st[:n], sub(0, n), off, lens)
            assert rules.same_bits(occ, full[0][:, :n]) and np.array_equal(win, full[1])


def test_scratch_passes_change_no_bit(ctx, monkeypatch):
    """the block sums go through bounded scratch: with a bound of a few cells the records, and for the long record the
    motifs, run in passes -- the same bits in both modes"""
    rng = np.random.default_rng(13)
    m = 12
    lengths = [int(x) for x in rng.integers(1, 1500, size=50)] + [40000] + [int(x) for x in rng.integers(1, 200, size=20)]
    codes, profile, off, lens = rules.stream(rng, lengths, np.float32, foreign=0.005)
    st = np.stack([rules.struct_table(rng, m, 0.5, 2.0) for _ in range(7)])
    sq = np.stack([orules.table(rng, m, 4, 0.5, 2.0) for _ in range(7)])
    want_s, want_j = check(ctx, codes, profile, off, lens, st), check(ctx, codes, profile, off, lens, st, sq)
    for cap in ("1", "50", "3000", "100000"):
        monkeypatch.setenv("PFMSCAN_OCC_SCRATCH_DOUBLES", cap)
        for want, tabs in ((want_s, None), (want_j, sq)):
            got = run(ctx, codes, profile, off, lens, st, tabs)
            assert rules.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_independent_of_order_batch_and_stream(ctx, dtype):
    """the same records in another order, split over two streams, named by a subset record table, and behind a first
    record of one row (28-byte rows: the second record starts at a row that is not 16-byte aligned)"""
    rng = np.random.default_rng(17)
    m = 12
    lengths = [int(x) for x in rng.integers(1, 4000, size=60)] + [33000]
    codes, profile, off, lens = rules.stream(rng, lengths, dtype, foreign=0.003)
    st = np.stack([rules.struct_table(rng, m, 0.5, 2.0) for _ in range(3)])
    sq = np.stack([orules.table(rng, m, 4, 0.5, 2.0) for _ in range(3)])
    recs = [(codes[o:o + n], profile[o:o + n]) for o, n in zip(off, lens)]

    def packed(order, lead=0):
        ln = np.asarray([recs[i][0].size for i in order], dtype=np.int64)
        of = np.zeros(ln.size, dtype=np.int64)
        of[1:] = np.cumsum(ln[:-1] + 1)
        of += lead                                                      # `lead` rows that belong to no record come first
        c = np.full(int((ln + 1).sum()) + lead, 7, dtype=np.uint8)
        p = np.full((c.size, 7), np.nan, dtype=dtype)
        for o, i in zip(of, order):
            c[o:o + recs[i][0].size] = recs[i][0]
            p[o:o + recs[i][0].size] = recs[i][1]
        return c, p, of, ln

    for tabs in (None, sq):
        base = check(ctx, codes, profile, off, lens, st, tabs)
        order = rng.permutation(len(recs))
        got = run(ctx, *packed(order), st, tabs)
        assert rules.same_bits(got[0], base[0][order]) and np.array_equal(got[1], base[1][order])
        cut = 37
        a = run(ctx, *packed(range(cut)), st, tabs)
        b = run(ctx, *packed(range(cut, len(recs))), st, tabs)
        assert rules.same_bits(np.concatenate([a[0], b[0]]), base[0]) and np.array_equal(np.concatenate([a[1], b[1]]), base[1])
        for lead in (1, 2, 3):                                          # every residue of the first row's byte offset mod 16
            got = run(ctx, *packed(range(len(recs)), lead), st, tabs)
            assert rules.same_bits(got[0], base[0]) and np.array_equal(got[1], base[1])
        some = np.sort(rng.choice(len(recs), size=20, replace=False))
        ctx.stage(codes, profile)
        part = ctx.occupancy_profile_staged(st, tabs, off[some], lens[some])
        assert rules.same_bits(part[0], base[0][some]) and np.array_equal(part[1], base[1][some])


@pytest.mark.parametrize("m", [1, 5, 12])
def test_one_hot_profile_equals_the_letter_occupancy(ctx, m):
    """rows that are one-hot in the structure letters: 1 * S + 0 * S ... = S exactly, so the structure-only occupancy is
    pfmscan_occupancy_staged's on the letter codes, bit for bit (finite tables; +0.0 cells allowed)"""
    rng = np.random.default_rng(41 + m)
    letters, off, lens = orules.stream(rng, [int(x) for x in rng.integers(1, 700, size=50)] + [9000], 7)
    S = rules.struct_table(rng, m)
    S[0, 3] = 0.0
    R = np.full((m, 8), np.nan)
    R[:, :7] = S
    ctx.stage(letters)
    want = ctx.occupancy_staged(R, 7, off, lens)
    for dtype in (np.float32, np.float64):
        ctx.stage(None, rules.one_hot(letters, dtype))
        got = ctx.occupancy_profile_staged(S, None, off, lens)
        assert rules.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_engine_method(ctx):
    from rnascan_amd import pack, scanner
    rng = np.random.default_rng(19)
    e = scanner.HipEngine(0)
    try:
        lens = (5, 300, 0, 77)
        stream = pack.pack([rng.integers(0, 4, size=n).astype(np.uint8) for n in lens], [rules.rows(rng, n) for n in lens])
        st, sq = rules.struct_table(rng, 6), orules.table(rng, 6)
        for tabs in (None, sq):
            occ, win = e.occupancy_profile(stream, st, tabs)
            want = rules.occupancy(stream.profile, stream.offsets, stream.lengths, st, stream.codes, tabs)
            assert rules.same_bits(occ, want[0]) and np.array_equal(win, want[1])
    finally:
        e.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dev_form_as_an_integrator_calls_it(ctx, dtype):
    """torch device tensors in and out, guard cells before and after EVERY buffer; equal to _staged; the guards unchanged"""
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(23)
    m, n_mo, G = 12, 5, 64                                              # G cells of guard: a multiple of 16 bytes for every dtype
    codes, profile, off, lens = rules.stream(rng, [int(x) for x in rng.integers(1, 2000, size=60)], dtype, foreign=0.004)
    st = np.stack([rules.struct_table(rng, m, 0.5, 2.0) for _ in range(n_mo)])
    sq = np.stack([orules.table(rng, m, 4, 0.5, 2.0) for _ in range(n_mo)])
    n_rec = len(off)
    code = _lib.PROFILE_F32 if dtype == np.float32 else _lib.PROFILE_F64

    def guarded(a, fill):
        flat = np.ascontiguousarray(a).reshape(-1)
        t = torch.full((G + flat.size + G,), fill, dtype=torch.from_numpy(flat[:1].copy()).dtype, device="cuda")
        t[G:G + flat.size] = torch.from_numpy(flat).cuda()
        return t

    d_codes, d_prof = guarded(codes, 7), guarded(profile, float("nan"))
    d_off, d_len = guarded(off, -1), guarded(lens, -1)
    inputs = [(d_codes, codes.reshape(-1), 7), (d_off, off, -1), (d_len, lens, -1)]
    for tabs in (None, sq):
        want = run(ctx, codes, profile, off, lens, st, tabs)
        for windows in (True, False):
            d_occ = torch.full((G + n_rec * n_mo + G,), -7.0, dtype=torch.float64, device="cuda")
            d_win = torch.full((G + n_rec + G,), -7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ctx.occupancy_profile_dev(st, tabs, d_codes.data_ptr() + G if tabs is not None else None, d_prof.data_ptr() + G * profile.itemsize,
                                      code, codes.size, d_off.data_ptr() + 8 * G, d_len.data_ptr() + 8 * G, n_rec,
                                      d_occ.data_ptr() + 8 * G, d_win.data_ptr() + 8 * G if windows else None)
            ctx.synchronize()
            occ, win = d_occ.cpu().numpy(), d_win.cpu().numpy()
            assert (occ[:G] == -7).all() and (occ[-G:] == -7).all() and (win[:G] == -7).all() and (win[-G:] == -7).all()
            assert rules.same_bits(occ[G:-G].reshape(n_rec, n_mo), want[0])
            assert np.array_equal(win[G:-G], want[1]) if windows else (win == -7).all()
            for t, host, fill in inputs:                                # the inputs and their guards are as they were
                back = t.cpu().numpy()
                assert (back[:G] == fill).all() and (back[-G:] == fill).all() and np.array_equal(back[G:-G], host)
            back = d_prof.cpu().numpy()
            assert np.isnan(back[:G]).all() and np.isnan(back[-G:]).all() and rules.same_bits(back[G:-G].astype(np.float64), profile.reshape(-1).astype(np.float64))


def test_bad_arguments_launch_nothing(ctx):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(29)
    codes, profile, off, lens = rules.stream(rng, [50, 60, 70], np.float32)
    d_codes, d_prof = torch.from_numpy(codes).cuda(), torch.from_numpy(profile).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    d_occ = torch.full((3, 2), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L, h, p = ctx._L, ctx._h, _lib._ptr
    S = np.ascontiguousarray(np.stack([rules.struct_table(rng, 8)] * 2))
    R = np.ascontiguousarray(np.stack([orules.table(rng, 8)] * 2))
    wide = np.ascontiguousarray(np.stack([rules.struct_table(rng, 65)] * 2))
    ptr = lambda t, shift=0: None if t is None else p(t.data_ptr() + shift)

    def dev(st=S, sq=None, n_mo=2, m=8, c=d_codes, prof=d_prof, dt=_lib.PROFILE_F32, n_pos=codes.size, o=d_off, ln=d_len, n_rec=3, out=d_occ,
            shift_prof=0, shift_codes=0):
        return L.pfmscan_occupancy_profile_dev(h, p(st), p(sq), n_mo, m, ptr(c, shift_codes), ptr(prof, shift_prof), dt, n_pos, ptr(o), ptr(ln),
                                               n_rec, ptr(out), None)
    assert dev(m=0) == _lib.E_BADSHAPE and dev(st=wide, m=65) == _lib.E_BADSHAPE
    assert dev(dt=_lib.PROFILE_NONE) == _lib.E_BADARG and dev(dt=3) == _lib.E_BADARG
    assert dev(st=None) == _lib.E_BADARG and dev(prof=None) == _lib.E_BADARG
    assert dev(sq=R, c=None) == _lib.E_BADARG                                       # joint mode without codes
    assert dev(o=None) == _lib.E_BADARG and dev(ln=None) == _lib.E_BADARG and dev(out=None) == _lib.E_BADARG
    assert dev(n_mo=-1) == _lib.E_BADARG and dev(n_rec=-1) == _lib.E_BADARG and dev(n_pos=-1) == _lib.E_BADARG
    assert dev(shift_prof=4) == _lib.E_BADSHAPE and dev(sq=R, shift_codes=1) == _lib.E_BADSHAPE
    assert dev(n_pos=codes.size - 2) == _lib.E_BADARG                               # the last record runs past n_pos
    swapped = torch.from_numpy(off[[1, 0, 2]].copy()).cuda()
    overlap = torch.from_numpy(np.asarray([0, 40, 112], dtype=np.int64)).cuda()
    torch.cuda.synchronize()
    assert dev(o=swapped) == _lib.E_BADARG and dev(o=overlap) == _lib.E_BADARG
    assert dev(n_mo=0) == 0 and dev(n_rec=0) == 0                                   # nothing to do: OK, nothing written
    ctx.synchronize()
    assert (d_occ.cpu().numpy() == -7).all()
    assert dev(c=None) == 0                                                         # structure only: the codes are not needed
    ctx.synchronize()
    assert rules.same_bits(d_occ.cpu().numpy(), rules.occupancy(profile, off, lens, S)[0])
    # the staged form
    out = np.zeros((3, 2))

    def staged(st=S, sq=None, n_mo=2, m=8, o=off, ln=lens, n_rec=3, res=out):
        return L.pfmscan_occupancy_profile_staged(h, p(st), p(sq), n_mo, m, p(o), p(ln), n_rec, p(res), None)
    ctx.stage(codes)                                                                # no profile staged
    assert staged() == _lib.E_BADARG
    ctx.stage(None, profile)                                                        # no codes staged
    assert staged(sq=R) == _lib.E_BADARG and staged() == 0
    ctx.stage(codes, profile)
    assert staged(m=0) == _lib.E_BADSHAPE and staged(st=wide, m=65) == _lib.E_BADSHAPE
    assert staged(st=None) == _lib.E_BADARG and staged(o=None) == _lib.E_BADARG and staged(ln=None) == _lib.E_BADARG and staged(res=None) == _lib.E_BADARG
    assert staged(n_mo=-1) == _lib.E_BADARG and staged(n_rec=-1) == _lib.E_BADARG
    assert staged(o=np.ascontiguousarray(off[[1, 0, 2]])) == _lib.E_BADARG and staged(ln=lens + 1000) == _lib.E_BADARG
    assert staged(n_mo=0) == 0 and staged(n_rec=0) == 0 and staged(sq=R) == 0
    assert rules.same_bits(out, rules.occupancy(profile, off, lens, S, codes, R)[0])
