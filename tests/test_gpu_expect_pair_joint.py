"""The expected letter-pair table of two code streams (k_exp_pair_blocks<true>, csrc/pfmscan_expect.hip; ABI 27) on the GPU
against the rules (tests/pair_joint_rules.py): every comparison is on the float64 bit patterns (NaN == NaN) plus equal Windows --
there is no tolerance in the contract.  The margins that come with the table are held to the rules and to the existing entry
points, the merged form to the Python integers of tests/expect_merge_rules.py, and the table of ones to the letter-pair counts of
the site profiles, an independent kernel."""
import itertools

import numpy as np
import pytest

import expect_merge_rules as mrules
import pair_joint_rules as rules
from test_gpu_occupancy import length_ladder

pytestmark = pytest.mark.gpu

MODES = (rules.RATIO, rules.POSTERIOR)
NAMES = ("exp_seq", "exp_struct", "exp_joint", "occ")


def stage(ctx, codes, codes2):
    ctx.stage(codes)
    ctx.stage_codes2(codes2)


def run(ctx, codes, codes2, off, lens, R, S, mode, **kw):
    stage(ctx, codes, codes2)
    return ctx.expect_pair_joint_staged(R, S, mode, off, lens, **kw)


def same(got, want):
    return (all(rules.same_bits(g, w) for g, w in zip(got[:4], want[:4])) and got[4].dtype == np.int64 and np.array_equal(got[4], want[4]))


def check(ctx, codes, codes2, off, lens, R, S, mode, want=None):
    got = run(ctx, codes, codes2, off, lens, R, S, mode)
    want = rules.expected(codes, codes2, off, lens, R, S, mode) if want is None else want
    for name, g, w in zip(NAMES, got, want):
        assert rules.same_bits(g, w), "%s bits differ at %s" % (name, np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])
    assert got[4].dtype == np.int64 and np.array_equal(got[4], want[4])
    return got


@pytest.mark.parametrize("m", [1, 8, 21, 64])
def test_record_lengths_and_widths(ctx, m):
    """blocks, level-1 groups and (at m = 8 only: the rules hold 39 m rows per window) level 2; m = 64 fills the strips"""
    rng = np.random.default_rng(400 + m)
    lengths = length_ladder(rng, m)
    if m != 8:
        lengths = [min(x, 1025 + m - 1) for x in lengths]             # the rules stay within seconds
    if m == 64:
        lengths = lengths[:-250]
    codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.001, foreign_struct=0.001, case=True)
    R, S = rules.table(rng, m, 4, 0.6, 1.7), rules.table(rng, m, 7, 0.6, 1.7)
    n_win = np.maximum(lens - m + 1, 0)
    for n in (0, 1, 31, 32, 33, 1023, 1024, 1025) + ((32768, 32769) if m == 8 else ()):
        assert (n_win == n).any()
    mode = rules.POSTERIOR if m != 8 else rules.RATIO
    got = check(ctx, codes, codes2, off, lens, R, S, mode)
    ej = got[2]
    assert ej.shape == (lens.size, 1, m, 4, 8) and (ej[n_win == 0] == 0).all() and not np.signbit(ej).any()
    assert (ej[..., 7] == 0).all() and np.isfinite(ej).all() and (ej[n_win > 0].sum(axis=(1, 2, 3, 4)) > 0).any()
    # the margins that come with the table are those of the existing entry point
    eq, es, occ, win = ctx.expect_pair_staged(R, S, mode, off, lens)
    assert rules.same_bits(eq, got[0]) and rules.same_bits(es, got[1]) and rules.same_bits(occ, got[3]) and np.array_equal(win, got[4])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [1, 8, 21])
def test_both_modes_and_foreign_codes_in_either_stream(ctx, m, mode):
    rng = np.random.default_rng(13 * m + mode)
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
        assert got[4][r] == 0 and got[3][r, 0] == 0 and (got[2][r] == 0).all() and not np.signbit(got[2][r]).any()
    plain = codes2.copy()                                             # a lower-case structure letter is its letter
    plain[plain != 7] &= 7
    assert (plain != codes2).any()
    assert same(run(ctx, codes, plain, off, lens, R, S, mode), got)


@pytest.mark.parametrize("mode", MODES)
def test_special_cells(ctx, mode):
    """0, inf, NaN, 0 x inf and an all-zero row, as test_gpu_expect_pair.py::test_special_cells builds them"""
    rng = np.random.default_rng(7 + mode)
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
        assert (got[2][:, 7] == 0).all() and not np.signbit(got[2][:, 7]).any()
        assert np.isnan(got[2][-1, 6]).any() and np.isnan(got[2][-1, 4]).any()


@pytest.fixture(scope="module")
def library():
    """a library across the occupancy's LDS chunk rule and its rules' answer, once"""
    rng = np.random.default_rng(15)
    m = 12
    chunk = rules.lds_chunk(m)
    n_max = chunk + 2
    lengths = [int(x) for x in rng.integers(1, 400, size=14)] + [2500] + [int(x) for x in rng.integers(1, 100, size=6)]
    codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.003, foreign_struct=0.003, case=True)
    Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(n_max)])
    Ss = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(n_max)])
    return chunk, codes, codes2, off, lens, Rs, Ss, rules.expected(codes, codes2, off, lens, Rs, Ss, rules.POSTERIOR)


def first(want, n):
    return tuple(x[:, :n] for x in want[:4]) + (want[4],)


def test_library_across_the_chunk_rule(ctx, library):
    chunk, codes, codes2, off, lens, Rs, Ss, want = library
    for n in (chunk - 1, chunk, chunk + 1):
        assert same(run(ctx, codes, codes2, off, lens, Rs[:n], Ss[:n], rules.POSTERIOR), first(want, n))


@pytest.mark.parametrize("cap", ["1", "50", "3000", "100000"])
def test_scratch_passes(ctx, library, monkeypatch, cap):
    """PFMSCAN_OCC_SCRATCH_DOUBLES small enough to force record passes and passes over the matrix rows: no bit changes"""
    _, codes, codes2, off, lens, Rs, Ss, want = library
    monkeypatch.setenv("PFMSCAN_OCC_SCRATCH_DOUBLES", cap)
    assert same(run(ctx, codes, codes2, off, lens, Rs[:3], Ss[:3], rules.POSTERIOR), first(want, 3))


def test_every_subset_of_the_outputs(ctx, library, monkeypatch):
    """what is asked for has the same bits, the rest is None; under a scratch cap that cuts the rows too"""
    _, codes, codes2, off, lens, Rs, Ss, want = library
    want = first(want, 3)
    margins = None
    for cap in (None, "700"):
        if cap:
            monkeypatch.setenv("PFMSCAN_OCC_SCRATCH_DOUBLES", cap)
        for asked in itertools.product((False, True), repeat=3):
            kw = dict(zip(("want_seq", "want_struct", "want_joint"), asked))
            if not any(asked):
                stage(ctx, codes, codes2)
                with pytest.raises(ValueError):
                    ctx.expect_pair_joint_staged(Rs[:3], Ss[:3], rules.POSTERIOR, off, lens, **kw)
                continue
            got = run(ctx, codes, codes2, off, lens, Rs[:3], Ss[:3], rules.POSTERIOR, **kw)
            for i, on in enumerate(asked):
                assert (rules.same_bits(got[i], want[i]) if on else got[i] is None), (asked, NAMES[i])
            assert rules.same_bits(got[3], want[3]) and np.array_equal(got[4], want[4])
        margins = ctx.expect_pair_staged(Rs[:3], Ss[:3], rules.POSTERIOR, off, lens)
        assert rules.same_bits(margins[0], want[0]) and rules.same_bits(margins[1], want[1]) and rules.same_bits(margins[2], want[3])


@pytest.mark.parametrize("mode", MODES)
def test_independent_of_order_batch_and_stream_offset(ctx, mode):
    rng = np.random.default_rng(19 + mode)
    m = 12
    lengths = [int(x) for x in rng.integers(1, 700, size=40)] + [2100]
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
    assert same(run(ctx, *packed(order), Rs, Ss, mode), tuple(x[order] for x in base))
    cut = 17
    a = run(ctx, *packed(range(cut)), Rs, Ss, mode)
    b = run(ctx, *packed(range(cut, len(recs))), Rs, Ss, mode)
    assert same(tuple(np.concatenate([x, y]) for x, y in zip(a, b)), base)
    for lead in (1, 2, 3):
        assert same(run(ctx, *packed(range(len(recs)), lead), Rs, Ss, mode), base)


def test_dev_form_as_an_integrator_calls_it(ctx):
    """torch device tensors in and out on the context's stream; equal to the rules; nothing written outside the outputs"""
    import torch
    rng = np.random.default_rng(31)
    m, n_mo = 12, 3
    codes, codes2, off, lens = rules.streams(rng, [int(x) for x in rng.integers(1, 600, size=25)], foreign_seq=0.003, foreign_struct=0.003, case=True)
    Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(n_mo)])
    Ss = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(n_mo)])
    want = rules.expected(codes, codes2, off, lens, Rs, Ss, rules.POSTERIOR)
    n_rec, guard, cells = len(off), 64, len(off) * n_mo * m * 8
    d_codes, d_codes2 = torch.from_numpy(codes).cuda(), torch.from_numpy(codes2).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    d_sq = torch.full((guard + cells + guard,), -7.0, dtype=torch.float64, device="cuda")
    d_st = torch.full((guard + cells + guard,), -7.0, dtype=torch.float64, device="cuda")
    d_jt = torch.full((guard + 4 * cells + guard,), -7.0, dtype=torch.float64, device="cuda")
    d_occ = torch.full((guard + n_rec * n_mo + guard,), -7.0, dtype=torch.float64, device="cuda")
    d_win = torch.full((guard + n_rec + guard,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.expect_pair_joint_dev(Rs, Ss, rules.POSTERIOR, d_codes.data_ptr(), d_codes2.data_ptr(), codes.size, d_off.data_ptr(), d_len.data_ptr(), n_rec,
                              d_sq.data_ptr() + 8 * guard, d_st.data_ptr() + 8 * guard, d_jt.data_ptr() + 8 * guard, d_occ.data_ptr() + 8 * guard,
                              d_win.data_ptr() + 8 * guard)
    ctx.synchronize()
    for t in (d_sq, d_st, d_jt, d_occ, d_win):
        x = t.cpu().numpy()
        assert (x[:guard] == -7).all() and (x[-guard:] == -7).all()
    shape = (n_rec, n_mo, m, 8)
    assert rules.same_bits(d_sq.cpu().numpy()[guard:-guard].reshape(shape), want[0])
    assert rules.same_bits(d_st.cpu().numpy()[guard:-guard].reshape(shape), want[1])
    assert rules.same_bits(d_jt.cpu().numpy()[guard:-guard].reshape(n_rec, n_mo, m, 4, 8), want[2])
    assert rules.same_bits(d_occ.cpu().numpy()[guard:-guard].reshape(n_rec, n_mo), want[3]) and np.array_equal(d_win.cpu().numpy()[guard:-guard], want[4])
    # the table alone, no occupancy, no Windows, ratio mode: the margins' buffers are left alone
    want = rules.expected(codes, codes2, off, lens, Rs, Ss, rules.RATIO)
    for t in (d_sq, d_st, d_jt):
        t.fill_(-7.0)
    torch.cuda.synchronize()
    ctx.expect_pair_joint_dev(Rs, Ss, rules.RATIO, d_codes.data_ptr(), d_codes2.data_ptr(), codes.size, d_off.data_ptr(), d_len.data_ptr(), n_rec,
                              None, None, d_jt.data_ptr() + 8 * guard)
    ctx.synchronize()
    x = d_jt.cpu().numpy()
    assert rules.same_bits(x[guard:-guard].reshape(n_rec, n_mo, m, 4, 8), want[2]) and (x[:guard] == -7).all() and (x[-guard:] == -7).all()
    assert (d_sq.cpu().numpy() == -7).all() and (d_st.cpu().numpy() == -7).all()


def test_bad_arguments_launch_nothing(ctx):
    import torch
    from rnascan_amd import _lib, expect
    rng = np.random.default_rng(37)
    codes, codes2, off, lens = rules.streams(rng, [50, 60, 70])
    d_codes, d_codes2 = torch.from_numpy(codes).cuda(), torch.from_numpy(codes2).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    d_sq = torch.full((3, 2, 8, 8), -7.0, dtype=torch.float64, device="cuda")
    d_st = torch.full((3, 2, 8, 8), -7.0, dtype=torch.float64, device="cuda")
    d_jt = torch.full((3, 2, 8, 4, 8), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L, h, p = ctx._L, ctx._h, _lib._ptr
    R, S = np.ascontiguousarray(np.stack([rules.table(rng, 8, 4)] * 2)), np.ascontiguousarray(np.stack([rules.table(rng, 8, 7)] * 2))
    wide = np.ascontiguousarray(np.stack([rules.table(rng, 65, 7)] * 2))
    ptr = lambda t, shift=0: p(t.data_ptr() + shift) if t is not None else None

    def dev(R=R, S=S, n_mo=2, m=8, mode=1, c=d_codes, c2=d_codes2, shift=0, shift2=0, n_pos=codes.size, o=d_off, ln=d_len, n_rec=3, sq=d_sq, st=d_st,
            jt=d_jt):
        return L.pfmscan_expect_pair_joint_dev(h, p(R), p(S), n_mo, m, mode, ptr(c, shift), ptr(c2, shift2), n_pos, ptr(o), ptr(ln), n_rec,
                                               ptr(sq), ptr(st), ptr(jt), None, None)
    assert dev(m=0) == _lib.E_BADSHAPE and dev(R=wide, S=wide, m=65) == _lib.E_BADSHAPE
    assert dev(shift=4) == _lib.E_BADSHAPE and dev(shift2=8) == _lib.E_BADSHAPE
    assert dev(mode=2) == _lib.E_BADARG and dev(mode=-1) == _lib.E_BADARG
    assert dev(R=None) == _lib.E_BADARG and dev(S=None) == _lib.E_BADARG and dev(c=None) == _lib.E_BADARG and dev(c2=None) == _lib.E_BADARG
    assert dev(o=None) == _lib.E_BADARG and dev(ln=None) == _lib.E_BADARG and dev(sq=None, st=None, jt=None) == _lib.E_BADARG
    assert dev(n_pos=codes.size - 2) == _lib.E_BADARG
    swapped = torch.from_numpy(off[[1, 0, 2]].copy()).cuda()
    torch.cuda.synchronize()
    assert dev(o=swapped) == _lib.E_BADARG
    assert dev(n_mo=0) == 0 and dev(n_rec=0) == 0                         # nothing to do: OK, nothing written
    ctx.synchronize()
    assert (d_sq.cpu().numpy() == -7).all() and (d_st.cpu().numpy() == -7).all() and (d_jt.cpu().numpy() == -7).all()
    assert dev() == 0
    ctx.synchronize()
    want = rules.expected(codes, codes2, off, lens, R, S, rules.POSTERIOR)
    assert rules.same_bits(d_sq.cpu().numpy(), want[0]) and rules.same_bits(d_st.cpu().numpy(), want[1]) and rules.same_bits(d_jt.cpu().numpy(), want[2])
    # the staged forms
    ctx.stage(codes)
    with pytest.raises(ValueError):
        ctx.expect_pair_joint_staged(R, S, 1, off, lens)                  # no codes2 staged
    ctx.stage_codes2(codes2)
    with pytest.raises(ValueError):
        ctx.expect_pair_joint_staged(R, S, 2, off, lens)
    with pytest.raises(ValueError):
        ctx.expect_pair_joint_staged(wide, wide, 1, off, lens)
    with pytest.raises(ValueError):
        ctx.expect_pair_joint_staged(R, S, 1, off[[1, 0, 2]], lens)
    acc = expect.new_acc(2, 4 * 8)
    with pytest.raises(ValueError):
        ctx.expect_pair_joint_merged_staged(R, S, 1, off, lens, None, None, None)
    with pytest.raises(ValueError):
        ctx.expect_pair_joint_merged_staged(R, S, 1, off, lens, None, None, expect.new_acc(2, 8))       # a table's accumulator has 4 m rows
    with pytest.raises(ValueError):
        ctx.expect_pair_joint_merged_staged(R, S, 3, off, lens, None, None, acc)
    assert not acc.any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [1, 12, 64])
def test_merged_form_against_the_integers(ctx, m, mode):
    """two batches added into one accumulator: the limbs are those of the Python integers over all records.  m = 64 is the
    widest table: 256 rows, k_exp_merge over 32 tiles of 64 cells (few records there: the integers are made in Python)"""
    from rnascan_amd import expect
    rng = np.random.default_rng(90 + m + mode)
    lengths = [int(x) + m - 1 for x in rng.integers(1, 300, size=70 if m < 64 else 34)] + [m - 1, 2000 if m < 64 else 700]
    codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.01, foreign_struct=0.01, case=True)
    R = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(3)])
    S = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(3)])
    S[2, 0, :7] = 0.0
    stage(ctx, codes, codes2)
    eq, es, ej, occ, win = ctx.expect_pair_joint_staged(R, S, mode, off, lens)
    accs = [expect.new_acc(3, m), expect.new_acc(3, m), expect.new_acc(3, 4 * m)]
    cut = 29
    occ2, win2 = [], []
    for a, b in ((0, cut), (cut, lens.size)):
        got = ctx.expect_pair_joint_merged_staged(R, S, mode, off[a:b], lens[a:b], *accs)
        assert all((bad == -1).all() for bad in got[:3])
        occ2.append(got[3])
        win2.append(got[4])
    for acc, exp in zip(accs, (eq, es, ej)):
        assert (acc == mrules.limbs_of(mrules.merge_ints(exp))).all()
    assert np.concatenate(occ2).tobytes() == occ.tobytes() and np.array_equal(np.concatenate(win2), win)
    only = expect.new_acc(3, 4 * m)
    got = ctx.expect_pair_joint_merged_staged(R, S, mode, off, lens, None, None, only)
    assert got[0] is None and got[1] is None and (got[2] == -1).all() and (only == accs[2]).all()
    # a non-finite cell that only the table's verdict can name a column for: records with letter 1 over letter 3 under column 0
    Rn = R.copy()
    Rn[1, 0, 1] = np.inf
    ej = ctx.expect_pair_joint_staged(Rn, S, mode, off, lens, want_seq=False, want_struct=False)[2]
    bad = ctx.expect_pair_joint_merged_staged(Rn, S, mode, off, lens, None, None, expect.new_acc(3, 4 * m))[2]
    assert bad.tolist() == mrules.bad(ej).tolist() and bad[1, 0] >= 0 and bad[0, 0] == -1


@pytest.mark.parametrize("mode", MODES)
def test_identities_against_the_single_stream_entry_points(ctx, mode):
    """a constant known letter in one stream: the table's one live slice is the OTHER stream's single-stream matrix, bit for bit"""
    rng = np.random.default_rng(23 + mode)
    for m in (8, 21):
        lengths = [int(x) + m - 1 for x in rng.integers(1, 1500, size=30)] + [m - 1, 4000]
        Rs = np.stack([rules.table(rng, m, 4, 0.6, 1.7) for _ in range(3)])
        Ss = np.stack([rules.table(rng, m, 7, 0.6, 1.7) for _ in range(3)])
        one = np.stack([rules.ones(m)] * 3)
        # identity 1: every record's structure string is one known letter (its own b0, some in lower case); S == 1.0
        codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.004, foreign_struct=0.0)
        b0 = rng.integers(0, 7, size=lens.size)
        for r in range(lens.size):
            codes2[off[r]:off[r] + lens[r]] = np.uint8(b0[r] | (8 if r % 3 == 0 else 0))
        got = run(ctx, codes, codes2, off, lens, Rs, one, mode)
        e, o, w = ctx.expect_staged(Rs, 4, mode, off, lens, 0)
        assert rules.same_bits(got[0], e) and rules.same_bits(got[3], o) and np.array_equal(got[4], w)
        for r in range(lens.size):
            assert rules.same_bits(got[2][r, :, :, :, b0[r]], e[r, :, :, :4])
            assert (np.delete(got[2][r], b0[r], axis=3) == 0).all() and not np.signbit(got[2][r]).any()
        # identity 2: every record's sequence is one known nucleotide a0; R == 1.0
        codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.0, foreign_struct=0.004, case=True)
        a0 = rng.integers(0, 4, size=lens.size)
        for r in range(lens.size):
            codes[off[r]:off[r] + lens[r]] = np.uint8(a0[r])
        got = run(ctx, codes, codes2, off, lens, one, Ss, mode)
        e, o, w = ctx.expect_staged(Ss, 7, mode, off, lens, 1)
        assert rules.same_bits(got[1], e) and rules.same_bits(got[3], o) and np.array_equal(got[4], w)
        for r in range(lens.size):
            assert rules.same_bits(got[2][r, :, :, a0[r], :], e[r])
            assert (np.delete(got[2][r], a0[r], axis=2) == 0).all()


def test_tables_of_ones_count_letter_pairs_as_the_site_profiles_do(ctx):
    """identity 3: R == S == 1.0, ratio weights, no foreign code -> every weight is 1.0 and the table is the integer count of
    letter pairs under every window: pfmscan_site_joint_staged with every window start as a hit, an independent kernel"""
    rng = np.random.default_rng(41)
    m = 8
    codes, codes2, off, lens = rules.streams(rng, list(range(1, 201)) + [3000], case=True)
    got = run(ctx, codes, codes2, off, lens, rules.ones(m), rules.ones(m), rules.RATIO)
    pos = np.concatenate([np.arange(o, o + max(n - m + 1, 0), dtype=np.int64) for o, n in zip(off, lens)])
    counts = ctx.site_joint_staged(pos, None, 1, off, lens, m)[0]
    assert counts.shape == (m, 8, 8) and int(counts.sum()) == pos.size * m and not counts[:, 4:].any() and not counts[:, :, 7].any()
    table = got[2][:, 0].sum(axis=0)                                      # integers below 2^53: the sum is exact in any order
    assert np.array_equal(table, counts[:, :4].astype(np.float64)) and np.array_equal(got[4], np.maximum(lens - m + 1, 0))
    assert np.array_equal(counts.astype(np.int64), rules.pair_counts(codes, codes2, off, lens, m))
    per_record = got[2][:, 0]
    assert np.array_equal(per_record, np.round(per_record)) and np.array_equal(per_record.sum(axis=(1, 2, 3)), m * np.maximum(lens - m + 1, 0))


def test_engine_methods(ctx):
    from rnascan_amd import expect, pack, scanner
    rng = np.random.default_rng(43)
    e = scanner.HipEngine(0)
    try:
        lens = (5, 300, 0, 77)
        stream = pack.pack([rng.integers(0, 4, size=n).astype(np.uint8) for n in lens])
        stream.codes2 = pack.pack([rng.integers(0, 7, size=n).astype(np.uint8) for n in lens]).codes
        R, S = rules.table(rng, 6, 4), rules.table(rng, 6, 7)
        for mode in MODES:
            want = rules.expected(stream.codes, stream.codes2, stream.offsets, stream.lengths, R, S, mode)
            assert same(e.expect_pair_joint(stream, R, S, mode), want)
            accs = [expect.new_acc(1, 6), expect.new_acc(1, 6), expect.new_acc(1, 24)]
            got = e.expect_pair_joint_merged(stream, R, S, mode, *accs)
            assert len(got) == 5 and rules.same_bits(got[3], want[3]) and (accs[2] == mrules.limbs_of(mrules.merge_ints(want[2]))).all()
    finally:
        e.close()
