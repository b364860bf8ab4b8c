"""k_expp_blocks (csrc/pfmscan_expect_profile.hip) on the GPU against the rules (tests/expect_profile_rules.py): every
comparison is on the float64 bit patterns (NaN == NaN) plus equal Windows -- there is no tolerance in the contract.  The
separator rows of every stream hold NaN: a kernel that read one as data would show it."""
import numpy as np
import pytest

import expect_profile_rules as rules
import occupancy_profile_rules as prules
import occupancy_rules as orules

pytestmark = pytest.mark.gpu

MODES = (rules.RATIO, rules.POSTERIOR)
FORMS = ("struct", "joint", "seq")                                     # which tables are given


def tables(form, st, sq):
    return (None if form == "seq" else st), (None if form == "struct" else sq)


def run(ctx, codes, profile, off, lens, st, sq, mode):
    ctx.stage(codes if sq is not None else None, profile)
    return ctx.expect_profile_staged(st, sq, mode, off, lens)


def where(got, want):
    return np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5]


def check(ctx, codes, profile, off, lens, st, sq, mode, want=None):
    got = run(ctx, codes, profile, off, lens, st, sq, mode)
    want = want or rules.expected(profile, off, lens, st, codes, sq, mode)
    assert rules.same_bits(got[2], want[2]) and got[3].dtype == np.int64 and np.array_equal(got[3], want[3])
    assert rules.same_bits(got[0], want[0]), "exp_struct bits differ at (record, motif, k, c) %s" % where(got[0], want[0])
    assert (got[1] is None) == (sq is None)
    if sq is not None:
        assert rules.same_bits(got[1], want[1]), "exp_seq bits differ at (record, motif, k, c) %s" % where(got[1], want[1])
    return got


def length_ladder(rng, m, top=True):
    """n_win at 0 (L = m - 3, m - 1), 1, 2, 31, 32, 33 (L = m .. m + 32), 255-257 (a run of 8 blocks and one window more),
    1024, 1025 and, with ``top``, 32 769 (a third level), among records of 1-3 blocks: a record ends inside a workgroup's run,
    a record straddles runs, and the record starts fall on every residue of the row size modulo 16 bytes"""
    lengths = []
    for n_win in (None, 0, 1, 2, 31, 32, 33, 255, 256, 257, 1024, 1025) + ((32769,) if top else ()):
        lengths += [int(x) + m - 1 for x in rng.integers(1, 97, size=3)]
        lengths.append(max(m - 3, 0) if n_win is None else n_win + m - 1)
    return lengths + [int(x) + m - 1 for x in rng.integers(1, 97, size=12)]


@pytest.fixture(scope="module")
def ladder():
    """the length ladder once per (width, row dtype): the stream and one table of each kind; the rules' answer once per
    (form, mode) of it"""
    streams, answers = {}, {}

    def get(m, dtype, form, mode):
        if (m, dtype) not in streams:
            rng = np.random.default_rng(500 + m)
            streams[(m, dtype)] = prules.stream(rng, length_ladder(rng, m, top=m == 12), dtype, foreign=0.002) + (
                prules.struct_table(rng, m, 0.5, 2.0), orules.table(rng, m, 4, 0.5, 2.0))
        codes, profile, off, lens, st, sq = streams[(m, dtype)]
        key = (m, dtype, form, mode)
        if key not in answers:
            a, b = tables(form, st, sq)
            answers[key] = rules.expected(profile, off, lens, a, codes, b, mode)
        return streams[(m, dtype)] + (answers[key],)
    return get


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_record_lengths_dtypes_forms_and_weights(ctx, ladder, dtype, form, mode):
    m = 12
    codes, profile, off, lens, st, sq, want = ladder(m, dtype, form, mode)
    n_win = np.maximum(lens - m + 1, 0)
    for n in (0, 1, 2, 31, 32, 33, 255, 256, 257, 1024, 1025, 32769):
        assert (n_win == n).any()
    row = 7 * np.dtype(dtype).itemsize
    assert set(((off * row) % 16).tolist()) == set(range(0, 16, 4 if dtype == np.float32 else 8))
    a, b = tables(form, st, sq)
    got = check(ctx, codes, profile, off, lens, a, b, mode, want)
    assert np.isfinite(got[0]).all() and (got[0][n_win == 0] == 0).all() and not np.signbit(got[0]).any()   # no separator row (NaN) was read
    assert (got[0][:, :, :, 7] == 0).all() and (got[0][:, :, :, :7] > 0).any()
    if form == "struct":
        assert np.array_equal(got[3], n_win)                            # every window inside a record has a term
    else:
        assert (got[3] <= n_win).all() and (got[3] < n_win).any() and (got[1][:, :, :, 4:] == 0).all()
    # occ and Windows are the occupancy's own bits
    ctx.stage(codes, profile)
    occ, win = ctx.occupancy_profile_staged(st, b, off, lens) if form != "seq" else ctx.occupancy_staged(sq, 4, off, lens)
    assert rules.same_bits(got[2], occ) and np.array_equal(got[3], win)
    if form == "seq":                                                   # ... and exp_seq is pfmscan_expect's matrix
        assert rules.same_bits(got[1], ctx.expect_staged(sq, 4, mode, off, lens)[0])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("m", [1, 2, 64])
def test_widths(ctx, ladder, m, form):
    for mode in MODES:
        codes, profile, off, lens, st, sq, want = ladder(m, np.float32, form, mode)
        check(ctx, codes, profile, off, lens, *tables(form, st, sq), mode, want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_base_case(ctx, dtype):
    """the case of which tests/test_expect_profile_cpu.py shows that a contracted w * r, the reversed column order, a shifted
    window and a division per window each give other bits"""
    codes, profile, off, lens, st, sq = prules.base_case(dtype=dtype)
    for form in FORMS:
        for mode in MODES:
            check(ctx, codes, profile, off, lens, *tables(form, st, sq), mode)


@pytest.mark.parametrize("form", FORMS)
def test_motif_counts(ctx, form):
    """1, 3, 9 and 33 motifs of one width in one call: motif k's matrices are the rules' for table k"""
    rng = np.random.default_rng(11)
    m = 5
    codes, profile, off, lens = prules.stream(rng, [int(x) for x in rng.integers(1, 120, size=8)] + [700], np.float32, foreign=0.01)
    st = np.stack([prules.struct_table(rng, m) for _ in range(33)])
    sq = np.stack([orules.table(rng, m) for _ in range(33)])
    a, b = tables(form, st, sq)
    for mode in MODES:
        want = rules.expected(profile, off, lens, a, codes, b, mode)
        for n in (33, 9, 3, 1):
            part = tuple(None if x is None else x[:, :n] for x in want[:3]) + (want[3],)
            check(ctx, codes, profile, off, lens, None if a is None else a[:n], None if b is None else b[:n], mode, part)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_values(ctx, dtype):
    """a record with a foreign code in every window (occ +0.0: every cell +0.0), a +inf table cell, a NaN, a negative and a
    -0.0 profile cell; columns of -0.0 under 1, 32, 33, 64, 1024 and 1056 windows: the sign of the zero sum is the rules'"""
    rng = np.random.default_rng(31)
    m = 6
    lengths = [90, 200, 40, 300, 77, m, m + 31, m + 32, m + 63, m + 1023, m + 1055, 500]
    codes, profile, off, lens = prules.stream(rng, lengths, dtype, foreign=0.005)
    codes[off[0]:off[0] + 90:4] = 7                                     # record 0: a foreign code in every window
    profile[off[1] + 5, 2] = np.nan
    profile[off[2] + 7, 4] = -0.25
    profile[off[3] + 9, 1] = -0.0
    for r in range(5, 11):
        profile[off[r]:off[r] + lens[r], 3] = -0.0                      # w * (-0.0) = -0.0 in every window of the record
        codes[off[r]:off[r] + lens[r]] &= 3                             # ... every one of which has a term
    profile[off[11]:off[11] + 500, 5] = -0.5
    st = np.stack([prules.struct_table(rng, m) for _ in range(3)])
    st[1, m - 1, 2] = np.inf                                            # rows with an exact zero in column 2: 0 x inf = NaN
    st[2, 0, 1] = 0.0
    sq = np.stack([orules.table(rng, m) for _ in range(3)])
    sq[2, 0, 2] = 0.0
    for form in FORMS:
        a, b = tables(form, st, sq)
        for mode in MODES:
            got = check(ctx, codes, profile, off, lens, a, b, mode)
            if form != "struct":
                assert got[3][0] == 0 and (got[2][0] == 0).all() and (got[0][0].view(np.uint64) == 0).all() and (got[1][0].view(np.uint64) == 0).all()
            zero = got[0][5:11, 0, :, 3]
            assert (zero == 0).all() and np.signbit(zero[[0, 1, 4]]).all() and not np.signbit(zero[[2, 3, 5]]).any()
            assert np.isnan(got[0][1, 0]).any()
            if form == "seq":
                assert (got[0][11, 0, :, 5] < 0).all()                  # positive weights over a column of -0.5
            if form != "seq":
                assert np.isnan(got[0][4, 1]).any() or np.isinf(got[0][4, 1]).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_weights_of_negative_zero(ctx, dtype):
    """joint form, ratio weights: every m-th row holds nothing but -0.0, so every window has exactly one marginal of -0.0 and
    a weight of -0.0.  exp_seq's cells are then sums of -0.0 and +0.0: a lone window and a column of one letter under 32 and
    1024 windows stay -0.0 (the first value of a block is copied, nothing is padded), 33 and 64 windows give +0.0"""
    rng = np.random.default_rng(37)
    m = 6
    n_wins = [1, 32, 33, 64, 1024, 200]
    codes, profile, off, lens = prules.stream(rng, [n + m - 1 for n in n_wins], dtype)
    for r in range(len(n_wins)):
        profile[off[r]:off[r] + lens[r]:m] = -0.0
        if r < 5:
            codes[off[r]:off[r] + lens[r]] = 2                          # one letter: column (k, 2) is -0.0 in every window
    st, sq = prules.struct_table(rng, m), orules.table(rng, m)
    ctx.stage(codes, profile)
    occ = ctx.occupancy_profile_staged(st, sq, off, lens)[0]
    res = {}
    for mode in MODES:
        got = res[mode] = run(ctx, codes, profile, off, lens, st, sq, mode)
        want = rules.expected(profile, off, lens, st, codes, sq, mode)
        assert rules.same_bits(got[0], want[0]), where(got[0], want[0])
        assert rules.same_bits(got[1], want[1]), where(got[1], want[1])
        assert np.array_equal(got[3], want[3]) and (got[2] == 0).all() and (got[1] == 0).all()
        # occ is pfmscan_occupancy_profile_*'s own: its bits, which are the rules' but for the sign of the zero of the record of
        # 64 windows (terms of nothing but -0.0 over two whole blocks: its levels 1 and up do not pad)
        assert rules.same_bits(got[2], occ)
        assert rules.same_bits(np.delete(got[2], 3, axis=0), np.delete(want[2], 3, axis=0))
    got = res[rules.RATIO]
    cell = got[1][:5, 0, :, 2]
    assert np.signbit(cell[[0, 1, 4]]).all() and not np.signbit(cell[[2, 3]]).any() and not np.signbit(got[1][:, 0, :, [0, 1, 3]]).any()
    assert np.signbit(got[0][0, 0]).any()
    assert (res[rules.POSTERIOR][1].view(np.uint64) == 0).all()         # occ == 0: every weight +0.0


def test_scratch_passes_change_no_bit(ctx, monkeypatch):
    """the block sums go through bounded scratch: with a bound of a few cells the records, and for the long record the matrix
    rows and motifs, run in passes -- the same bits in every form"""
    rng = np.random.default_rng(13)
    m = 8
    lengths = [int(x) for x in rng.integers(1, 700, size=20)] + [5000] + [int(x) for x in rng.integers(1, 200, size=8)]
    codes, profile, off, lens = prules.stream(rng, lengths, np.float32, foreign=0.005)
    st = np.stack([prules.struct_table(rng, m, 0.5, 2.0) for _ in range(3)])
    sq = np.stack([orules.table(rng, m, 4, 0.5, 2.0) for _ in range(3)])
    for form in FORMS:
        a, b = tables(form, st, sq)
        for mode in MODES:
            want = check(ctx, codes, profile, off, lens, a, b, mode)
            for cap in ("1", "3000", "7000", "100000"):               # 157 blocks in the long record: 1, 1 or 2, 4 or 6 and all 24 matrix rows per pass
                monkeypatch.setenv("PFMSCAN_OCC_SCRATCH_DOUBLES", cap)
                assert rules.same(run(ctx, codes, profile, off, lens, a, b, mode), want)
            monkeypatch.delenv("PFMSCAN_OCC_SCRATCH_DOUBLES")


def test_engine_method(ctx):
    from rnascan_amd import _lib, pack, scanner
    rng = np.random.default_rng(19)
    e = scanner.HipEngine(0)
    try:
        lens = (5, 300, 0, 77)
        stream = pack.pack([rng.integers(0, 4, size=n).astype(np.uint8) for n in lens], [prules.rows(rng, n) for n in lens])
        st, sq = prules.struct_table(rng, 6), orules.table(rng, 6)
        for form in FORMS:
            a, b = tables(form, st, sq)
            for mode, name in ((rules.RATIO, _lib.EXPECT_RATIO), (rules.POSTERIOR, _lib.EXPECT_POSTERIOR)):
                got = e.expect_profile(stream, a, b, name)
                assert rules.same(got, rules.expected(stream.profile, stream.offsets, stream.lengths, a, stream.codes, b, mode))
    finally:
        e.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dev_form_as_an_integrator_calls_it(ctx, dtype):
    """torch device tensors in and out, guard cells around every output; a subset record table; equal to _staged; occ and
    Windows are pfmscan_occupancy_profile_dev's bits (pfmscan_expect_dev's in the sequence-only form); the outputs optional"""
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(23)
    m, n_mo, G = 12, 3, 64
    codes, profile, off, lens = prules.stream(rng, [int(x) for x in rng.integers(1, 2000, size=40)], dtype, foreign=0.004)
    st = np.stack([prules.struct_table(rng, m, 0.5, 2.0) for _ in range(n_mo)])
    sq = np.stack([orules.table(rng, m, 4, 0.5, 2.0) for _ in range(n_mo)])
    some = np.sort(rng.choice(len(off), size=25, replace=False))
    off, lens = np.ascontiguousarray(off[some]), np.ascontiguousarray(lens[some])
    n_rec = len(off)
    code = _lib.PROFILE_F32 if dtype == np.float32 else _lib.PROFILE_F64
    d_codes, d_prof = torch.from_numpy(codes).cuda(), torch.from_numpy(profile).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    cells = n_rec * n_mo * m * 8

    def buffers():
        return (torch.full((G + cells + G,), -7.0, dtype=torch.float64, device="cuda"), torch.full((G + cells + G,), -7.0, dtype=torch.float64, device="cuda"),
                torch.full((G + n_rec * n_mo + G,), -7.0, dtype=torch.float64, device="cuda"), torch.full((G + n_rec + G,), -7, dtype=torch.int64, device="cuda"))

    for form in FORMS:
        a, b = tables(form, st, sq)
        for mode in MODES:
            want = run(ctx, codes, profile, off, lens, a, b, mode)
            d_st, d_sq, d_occ, d_win = buffers()
            torch.cuda.synchronize()
            ctx.expect_profile_dev(a, b, mode, d_codes.data_ptr() if b is not None else None, d_prof.data_ptr(), code, codes.size, d_off.data_ptr(),
                                   d_len.data_ptr(), n_rec, d_st.data_ptr() + 8 * G, d_sq.data_ptr() + 8 * G if b is not None else None,
                                   d_occ.data_ptr() + 8 * G, d_win.data_ptr() + 8 * G)
            ctx.synchronize()
            out = [x.cpu().numpy() for x in (d_st, d_sq, d_occ, d_win)]
            for x in out:
                assert (x[:G] == -7).all() and (x[-G:] == -7).all()
            got = (out[0][G:-G].reshape(n_rec, n_mo, m, 8), out[1][G:-G].reshape(n_rec, n_mo, m, 8) if b is not None else None,
                   out[2][G:-G].reshape(n_rec, n_mo), out[3][G:-G])
            assert rules.same(got, want)
            if b is None:
                assert (out[1] == -7).all()
            # occ and Windows against the occupancy's own _dev entry points
            o_occ = torch.full((n_rec, n_mo), -7.0, dtype=torch.float64, device="cuda")
            o_win = torch.full((n_rec,), -7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            if form == "seq":
                ctx.occupancy_dev(sq, 4, d_codes.data_ptr(), codes.size, d_off.data_ptr(), d_len.data_ptr(), n_rec, o_occ.data_ptr(), o_win.data_ptr())
            else:
                ctx.occupancy_profile_dev(st, b, d_codes.data_ptr() if b is not None else None, d_prof.data_ptr(), code, codes.size, d_off.data_ptr(),
                                          d_len.data_ptr(), n_rec, o_occ.data_ptr(), o_win.data_ptr())
            ctx.synchronize()
            assert rules.same_bits(o_occ.cpu().numpy(), got[2]) and np.array_equal(o_win.cpu().numpy(), got[3])
            if form == "seq":
                e_exp = torch.full((n_rec, n_mo, m, 8), -7.0, dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                ctx.expect_dev(sq, 4, mode, d_codes.data_ptr(), codes.size, d_off.data_ptr(), d_len.data_ptr(), n_rec, e_exp.data_ptr())
                ctx.synchronize()
                assert rules.same_bits(e_exp.cpu().numpy(), got[1])
            # without the optional outputs
            d_st, _, _, _ = buffers()
            torch.cuda.synchronize()
            ctx.expect_profile_dev(a, b, mode, d_codes.data_ptr() if b is not None else None, d_prof.data_ptr(), code, codes.size, d_off.data_ptr(),
                                   d_len.data_ptr(), n_rec, d_st.data_ptr() + 8 * G)
            ctx.synchronize()
            assert rules.same_bits(d_st.cpu().numpy()[G:-G].reshape(n_rec, n_mo, m, 8), want[0])


def test_bad_arguments_launch_nothing(ctx):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(29)
    codes, profile, off, lens = prules.stream(rng, [50, 60, 70], np.float32)
    d_codes, d_prof = torch.from_numpy(codes).cuda(), torch.from_numpy(profile).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    d_st = torch.full((3, 2, 8, 8), -7.0, dtype=torch.float64, device="cuda")
    d_sq = torch.full((3, 2, 8, 8), -7.0, dtype=torch.float64, device="cuda")
    d_occ = torch.full((3, 2), -7.0, dtype=torch.float64, device="cuda")
    d_win = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L, h, p = ctx._L, ctx._h, _lib._ptr
    S = np.ascontiguousarray(np.stack([prules.struct_table(rng, 8)] * 2))
    R = np.ascontiguousarray(np.stack([orules.table(rng, 8)] * 2))
    wide = np.ascontiguousarray(np.stack([prules.struct_table(rng, 65)] * 2))
    ptr = lambda t, shift=0: None if t is None else p(t.data_ptr() + shift)

    def dev(st=S, sq=R, n_mo=2, m=8, mode=1, c=d_codes, prof=d_prof, dt=_lib.PROFILE_F32, n_pos=codes.size, o=d_off, ln=d_len, n_rec=3, out=d_st,
            out_seq=d_sq, shift_prof=0, shift_codes=0):
        return L.pfmscan_expect_profile_dev(h, p(st), p(sq), n_mo, m, mode, ptr(c, shift_codes), ptr(prof, shift_prof), dt, n_pos, ptr(o), ptr(ln),
                                            n_rec, ptr(out), ptr(out_seq), ptr(d_occ), ptr(d_win))
    assert dev(m=0) == _lib.E_BADSHAPE and dev(st=wide, m=65) == _lib.E_BADSHAPE
    assert dev(dt=_lib.PROFILE_NONE) == _lib.E_BADARG and dev(dt=3) == _lib.E_BADARG and dev(mode=2) == _lib.E_BADARG and dev(mode=-1) == _lib.E_BADARG
    assert dev(st=None, sq=None, out_seq=None) == _lib.E_BADARG          # both tables NULL
    assert dev(sq=None) == _lib.E_BADARG                                 # exp_seq without seq_tables
    assert dev(c=None) == _lib.E_BADARG and dev(prof=None) == _lib.E_BADARG and dev(st=None, prof=None) == _lib.E_BADARG
    assert dev(o=None) == _lib.E_BADARG and dev(ln=None) == _lib.E_BADARG and dev(out=None) == _lib.E_BADARG
    assert dev(n_mo=-1) == _lib.E_BADARG and dev(n_rec=-1) == _lib.E_BADARG and dev(n_pos=-1) == _lib.E_BADARG
    assert dev(shift_prof=4) == _lib.E_BADSHAPE and dev(shift_codes=1) == _lib.E_BADSHAPE
    assert dev(n_pos=codes.size - 2) == _lib.E_BADARG                    # the last record runs past n_pos
    swapped = torch.from_numpy(off[[1, 0, 2]].copy()).cuda()
    overlap = torch.from_numpy(np.asarray([0, 40, 112], dtype=np.int64)).cuda()
    longer = torch.from_numpy(lens + 1000).cuda()
    torch.cuda.synchronize()
    assert dev(o=swapped) == _lib.E_BADARG and dev(o=overlap) == _lib.E_BADARG and dev(ln=longer) == _lib.E_BADARG
    assert dev(n_mo=0) == 0 and dev(n_rec=0) == 0                        # nothing to do: OK, nothing written
    ctx.synchronize()
    for t in (d_st, d_sq, d_occ, d_win):
        assert (t.cpu().numpy() == -7).all()
    assert dev() == 0
    ctx.synchronize()
    want = rules.expected(profile, off, lens, S, codes, R, rules.POSTERIOR)
    assert rules.same((d_st.cpu().numpy(), d_sq.cpu().numpy(), d_occ.cpu().numpy(), d_win.cpu().numpy()), want)
    assert dev(sq=None, out_seq=None, c=None) == 0                       # structure only: the codes are not needed
    ctx.synchronize()
    assert rules.same_bits(d_st.cpu().numpy(), rules.expected(profile, off, lens, S, mode=rules.POSTERIOR)[0])
    # the staged form
    ctx.stage(codes)                                                     # no profile staged
    with pytest.raises(ValueError):
        ctx.expect_profile_staged(S, None, rules.POSTERIOR, off, lens)
    ctx.stage(None, profile)                                             # no codes staged
    with pytest.raises(ValueError):
        ctx.expect_profile_staged(S, R, rules.POSTERIOR, off, lens)
    assert rules.same(ctx.expect_profile_staged(S, None, rules.RATIO, off, lens), rules.expected(profile, off, lens, S, mode=rules.RATIO))
    ctx.stage(codes, profile)
    for bad in ((off[[1, 0, 2]], lens), (off, lens + 1000)):
        with pytest.raises(ValueError):
            ctx.expect_profile_staged(S, R, rules.POSTERIOR, *bad)
    with pytest.raises(ValueError):
        ctx.expect_profile_staged(S, R, 2, off, lens)
    out = np.full((3, 2, 8, 8), -7.0)
    assert L.pfmscan_expect_profile_staged(h, p(S), None, 2, 8, 1, p(off), p(lens), 3, p(out), p(out), None, None) == _lib.E_BADARG
    assert (out == -7).all()
