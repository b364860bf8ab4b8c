"""k_expp_blocks<.., JOINT> (csrc/pfmscan_expect_profile.hip) on the GPU against the rules
(tests/expect_profile_joint_rules.py): every comparison is on the float64 bit patterns (NaN == NaN) plus equal Windows -- there
is no tolerance in the contract.  The separator rows of every stream hold NaN: a kernel that read one as data would show it."""
import numpy as np
import pytest

import expect_merge_rules as mrules
import expect_profile_joint_rules as rules
import occupancy_profile_rules as prules
import occupancy_rules as orules
from test_gpu_expect_profile import length_ladder

pytestmark = pytest.mark.gpu

MODES = (rules.RATIO, rules.POSTERIOR)
FORMS = ("joint", "seq")                                               # the forms that have codes


def tables(form, st, sq):
    return (None if form == "seq" else st), sq


def run(ctx, codes, profile, off, lens, st, sq, mode, **want):
    ctx.stage(codes, profile)
    return ctx.expect_profile_joint_staged(st, sq, mode, off, lens, **want)


def where(got, want):
    return np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5]


def check(ctx, codes, profile, off, lens, st, sq, mode, want=None):
    got = run(ctx, codes, profile, off, lens, st, sq, mode)
    want = want or rules.expected(profile, codes, off, lens, sq, st, mode)
    assert rules.same_bits(got[3], want[3]) and got[4].dtype == np.int64 and np.array_equal(got[4], want[4])
    assert got[2].shape == want[2].shape
    assert rules.same_bits(got[2], want[2]), "exp_joint bits differ at (record, motif, k, a, c) %s" % where(got[2], want[2])
    assert rules.same_bits(got[0], want[0]), "exp_struct bits differ at (record, motif, k, c) %s" % where(got[0], want[0])
    assert rules.same_bits(got[1], want[1]), "exp_seq bits differ at (record, motif, k, c) %s" % where(got[1], want[1])
    return got


@pytest.fixture(scope="module")
def ladder():
    """the length ladder once per (width, row dtype): the stream and one table of each kind; the rules' answer once per
    (form, mode) of it"""
    streams, answers = {}, {}

    def get(m, dtype, form, mode):
        if (m, dtype) not in streams:
            rng = np.random.default_rng(700 + m)
            streams[(m, dtype)] = prules.stream(rng, length_ladder(rng, m, top=m == 12), dtype, foreign=0.002) + (
                prules.struct_table(rng, m, 0.5, 2.0), orules.table(rng, m, 4, 0.5, 2.0))
        codes, profile, off, lens, st, sq = streams[(m, dtype)]
        key = (m, dtype, form, mode)
        if key not in answers:
            a, b = tables(form, st, sq)
            answers[key] = rules.expected(profile, codes, off, lens, b, a, mode)
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
    ej = got[2]
    assert np.isfinite(ej).all() and (ej[n_win == 0] == 0).all() and not np.signbit(ej).any()   # no separator row (NaN) was read
    assert (ej[..., 7] == 0).all() and (ej[..., :7] > 0).any() and (got[4] < n_win).any()
    # the existing entry point returns the same margins, occupancy and Windows
    ctx.stage(codes, profile)
    old = ctx.expect_profile_staged(a, b, mode, off, lens)
    assert rules.same_bits(old[0], got[0]) and rules.same_bits(old[1], got[1]) and rules.same_bits(old[2], got[3]) and np.array_equal(old[3], got[4])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("m", [1, 2, 64])
def test_widths(ctx, ladder, m, form):
    for mode in MODES:
        codes, profile, off, lens, st, sq, want = ladder(m, np.float32, form, mode)
        check(ctx, codes, profile, off, lens, *tables(form, st, sq), mode, want)


@pytest.mark.parametrize("form", FORMS)
def test_motif_counts_and_output_subsets(ctx, form):
    """1, 3 and 9 motifs of one width in one call: motif k's table is the rules' for table k; every subset of the three outputs
    gives the bits of all three"""
    rng = np.random.default_rng(11)
    m = 5
    codes, profile, off, lens = prules.stream(rng, [int(x) for x in rng.integers(1, 120, size=8)] + [700], np.float32, foreign=0.01)
    st = np.stack([prules.struct_table(rng, m) for _ in range(9)])
    sq = np.stack([orules.table(rng, m) for _ in range(9)])
    a, b = tables(form, st, sq)
    for mode in MODES:
        want = rules.expected(profile, codes, off, lens, b, a, mode)
        for n in (9, 3, 1):
            part = tuple(x[:, :n] for x in want[:4]) + (want[4],)
            check(ctx, codes, profile, off, lens, None if a is None else a[:n], b[:n], mode, part)
        for mask in range(1, 7):                                          # 7: all three, above
            ws, wq, wj = bool(mask & 1), bool(mask & 2), bool(mask & 4)
            got = run(ctx, codes, profile, off, lens, a, b, mode, want_struct=ws, want_seq=wq, want_joint=wj)
            picked = tuple(w if on else None for w, on in zip(want[:3], (ws, wq, wj))) + want[3:]
            assert rules.same(got, picked), mask


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_values(ctx, dtype):
    """a record with a foreign code in every window (occ +0.0: every cell +0.0), a +inf table cell, a NaN, a negative and a
    -0.0 profile cell; columns of -0.0 under 1, 32, 33, 64, 1024 and 1056 windows of one nucleotide: the sign of the zero sum is
    the rules'"""
    rng = np.random.default_rng(31)
    m = 6
    lengths = [90, 200, 40, 300, 77, m, m + 31, m + 32, m + 63, m + 1023, m + 1055, 500]
    codes, profile, off, lens = prules.stream(rng, lengths, dtype, foreign=0.005)
    codes[off[0]:off[0] + 90:4] = 7                                     # record 0: a foreign code in every window
    profile[off[1] + 5, 2] = np.nan
    profile[off[2] + 7, 4] = -0.25
    profile[off[3] + 9, 1] = -0.0
    profile[off[4] + 11, 6] = np.inf
    profile[off[4] + 30, 0] = -np.inf
    for r in range(5, 11):
        profile[off[r]:off[r] + lens[r], 3] = -0.0                      # w * (-0.0) = -0.0 in every window of the record
        codes[off[r]:off[r] + lens[r]] = 2                              # ... every one of which has a term and the letter 2
    profile[off[11]:off[11] + 500, 5] = -0.5
    st = np.stack([prules.struct_table(rng, m) for _ in range(3)])
    st[1, m - 1, 2] = np.inf
    st[2, 0, 1] = 0.0
    sq = np.stack([orules.table(rng, m) for _ in range(3)])
    sq[2, 0, 2] = 0.0
    for form in FORMS:
        a, b = tables(form, st, sq)
        for mode in MODES:
            got = check(ctx, codes, profile, off, lens, a, b, mode)
            ej = got[2]
            assert got[4][0] == 0 and (got[3][0] == 0).all() and (ej[0].view(np.uint64) == 0).all()
            zero = ej[5:11, 0, :, 2, 3]
            assert (zero == 0).all() and np.signbit(zero[[0, 1, 4]]).all() and not np.signbit(zero[[2, 3, 5]]).any()
            assert (ej[5:11, 0, :, [0, 1, 3]].view(np.uint64) == 0).all()  # the other nucleotides: +0.0
            assert np.isnan(ej[1, 0]).any() and (np.isnan(ej[4, 0]).any() or np.isinf(ej[4, 0]).any())
            if form == "seq":
                assert (ej[11, 0, :, :, 5] <= 0).all() and (ej[11, 0, :, :, 5] < 0).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_weights_of_negative_zero(ctx, dtype):
    """joint form, ratio weights: every m-th row holds nothing but -0.0, so every window has a weight of -0.0; the table's cells
    are sums of +-0.0 whose sign is the rules'.  Posterior: occ == 0, every cell +0.0"""
    rng = np.random.default_rng(37)
    m = 6
    n_wins = [1, 32, 33, 64, 1024, 200]
    codes, profile, off, lens = prules.stream(rng, [n + m - 1 for n in n_wins], dtype)
    for r in range(len(n_wins)):
        profile[off[r]:off[r] + lens[r]:m] = -0.0
        if r < 5:
            codes[off[r]:off[r] + lens[r]] = 2
    st, sq = prules.struct_table(rng, m), orules.table(rng, m)
    for mode in MODES:
        got = run(ctx, codes, profile, off, lens, st, sq, mode)
        want = rules.expected(profile, codes, off, lens, sq, st, mode)
        assert rules.same_bits(got[2], want[2]), where(got[2], want[2])
        assert rules.same_bits(got[0], want[0]) and rules.same_bits(got[1], want[1]) and np.array_equal(got[4], want[4])
        assert (got[2] == 0).all() and (got[3] == 0).all()
        if mode == rules.RATIO:
            assert np.signbit(got[2][:, 0, :, 2]).any()
        assert not np.signbit(got[2][:5, 0, :, [0, 1, 3]]).any()         # the other nucleotides: nothing selected, +0.0


def test_scratch_passes_change_no_bit(ctx, monkeypatch):
    """the block sums go through bounded scratch: with a bound of a few cells the records, and for the long record the matrix
    rows and motifs, run in passes -- the same bits in every form, with the table alone and with all three"""
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
            for cap in ("1", "3000", "7000", "100000"):               # 157 blocks in the long record: rows and records are cut
                monkeypatch.setenv("PFMSCAN_OCC_SCRATCH_DOUBLES", cap)
                assert rules.same(run(ctx, codes, profile, off, lens, a, b, mode), want), cap
                alone = run(ctx, codes, profile, off, lens, a, b, mode, want_struct=False, want_seq=False)
                assert rules.same(alone, (None, None) + tuple(want[2:])), cap
            monkeypatch.delenv("PFMSCAN_OCC_SCRATCH_DOUBLES")


def test_record_order_batch_split_and_stream_offset(ctx):
    rng = np.random.default_rng(17)
    m = 7
    lengths = [int(x) for x in rng.integers(1, 400, size=14)] + [1100]
    codes, profile, off, lens = prules.stream(rng, lengths, np.float32, foreign=0.005)
    st, sq = prules.struct_table(rng, m), orules.table(rng, m)
    for mode in MODES:
        want = check(ctx, codes, profile, off, lens, st, sq, mode)
        # a batch of some records, in the stream's order: the bits of the same records in the whole call
        for some in (np.arange(0, 15, 2), np.arange(5, 15), np.asarray([14])):
            got = run(ctx, codes, profile, np.ascontiguousarray(off[some]), np.ascontiguousarray(lens[some]), st, sq, mode)
            assert rules.same(got, tuple(x[some] for x in want))
        # the records in another order at other offsets of another stream (3 rows in front: other residues of 16 bytes)
        perm = rng.permutation(15)
        c2, p2, o2 = [np.full(3, 7, dtype=np.uint8)], [np.full((3, 7), np.nan, dtype=np.float32)], []
        at = 3
        for r in perm:
            o2.append(at)
            c2 += [codes[off[r]:off[r] + lens[r]], np.full(1, 7, dtype=np.uint8)]
            p2 += [profile[off[r]:off[r] + lens[r]], np.full((1, 7), np.nan, dtype=np.float32)]
            at += int(lens[r]) + 1
        got = run(ctx, np.concatenate(c2), np.ascontiguousarray(np.concatenate(p2)), np.asarray(o2, dtype=np.int64), np.ascontiguousarray(lens[perm]), st, sq, mode)
        assert rules.same(got, tuple(x[perm] for x in want))


def test_engine_methods(ctx):
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
                want = rules.expected(stream.profile, stream.codes, stream.offsets, stream.lengths, b, a, mode)
                assert rules.same(e.expect_profile_joint(stream, a, b, name), want)
                accs = [np.zeros((1, _lib.SITE_LIMBS, rows * 8), dtype=np.uint64) for rows in (6, 6, 24)]
                bads = e.expect_profile_joint_merged(stream, a, b, name, *accs)
                for acc, bad, w in zip(accs, bads[:3], want[:3]):
                    assert np.array_equal(acc, mrules.limbs_of(mrules.merge_ints(w.reshape(w.shape[:2] + (-1, 8))))) and (bad == -1).all()
                assert rules.same_bits(bads[3], want[3]) and np.array_equal(bads[4], want[4])
    finally:
        e.close()


@pytest.mark.parametrize("m", [1, 12, 64])
def test_merged_form_against_the_exact_integers(ctx, m):
    """the records added up on the device: the accumulators are the rules' exact integers of the rules' matrices, the verdicts
    theirs; a second call adds to the first; any accumulator may be left out"""
    from rnascan_amd import _lib
    rng = np.random.default_rng(43 + m)
    lengths = [int(x) + m - 1 for x in rng.integers(1, 300, size=9)] + [m - 1, 1025 + m - 1]
    codes, profile, off, lens = prules.stream(rng, lengths, np.float32, foreign=0.004)
    profile[off[4] + m - 1, 2] = np.nan                                 # record 4: a non-finite cell
    profile[off[6]:off[6] + lens[6], 5] = -0.5                          # record 6: negative cells
    n_mo = 2
    st = np.stack([prules.struct_table(rng, m, 0.7, 1.4) for _ in range(n_mo)])
    sq = np.stack([orules.table(rng, m, 4, 0.7, 1.4) for _ in range(n_mo)])
    ctx.stage(codes, profile)
    for form in FORMS:
        a, b = tables(form, st, sq)
        for mode in MODES:
            want = rules.expected(profile, codes, off, lens, b, a, mode)
            flat = [w.reshape(w.shape[:2] + (-1, 8)) for w in want[:3]]
            accs = [np.zeros((n_mo, _lib.SITE_LIMBS, rows * 8), dtype=np.uint64) for rows in (m, m, 4 * m)]
            got = ctx.expect_profile_joint_merged_staged(a, b, mode, off, lens, *accs)
            for acc, bad, w in zip(accs, got[:3], flat):
                assert np.array_equal(acc, mrules.limbs_of(mrules.merge_ints(w))) and np.array_equal(bad, mrules.bad(w))
            assert rules.same_bits(got[3], want[3]) and np.array_equal(got[4], want[4])
            assert (got[2][:, 0] == 4).all() and (got[2][:, 1] == 6).all() and np.array_equal(got[0], got[2])
            again = ctx.expect_profile_joint_merged_staged(a, b, mode, off, lens, None, None, accs[2])
            assert again[0] is None and again[1] is None and np.array_equal(accs[2], mrules.limbs_of(2 * mrules.merge_ints(flat[2])))


# ---- the three identities on the device ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_identity_1_a_constant_nucleotide(ctx, dtype):
    rng = np.random.default_rng(51)
    m = 8
    codes, profile, off, lens = prules.stream(rng, length_ladder(rng, m, top=False), dtype)
    a0 = rng.integers(0, 4, size=lens.size)
    for r in range(lens.size):
        codes[off[r]:off[r] + lens[r]] = np.uint8(a0[r] | (8 if r % 2 else 0))
    st, sq = prules.struct_table(rng, m), orules.table(rng, m)
    for form in FORMS:
        a, b = tables(form, st, sq)
        for mode in MODES:
            es, eq, ej, occ, win = run(ctx, codes, profile, off, lens, a, b, mode)
            for r in range(lens.size):
                assert rules.same_bits(ej[r, 0, :, a0[r], :], es[r, 0]), r
                assert (np.delete(ej[r, 0], a0[r], axis=1).view(np.uint64) == 0).all(), r
            assert (ej > 0).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_identity_2_one_hot_rows_against_the_letter_pair_kernel(ctx, dtype):
    """rows with a single 1.0, finite positive tables, identity column order: the table is bit for bit the table
    pfmscan_expect_pair_joint_* makes of the letter codes argmax(row) -- an independent kernel"""
    rng = np.random.default_rng(53)
    m = 8
    lengths = length_ladder(rng, m, top=False)
    letters, off, lens = orules.stream(rng, lengths, 7, case=False)
    codes, _, off2, lens2 = prules.stream(rng, lengths, dtype, foreign=0.004)
    assert np.array_equal(off, off2) and np.array_equal(lens, lens2)
    profile = prules.one_hot(letters, dtype)
    codes2 = letters.copy()
    codes2[codes2 > 6] = 7
    st, sq = prules.struct_table(rng, m), orules.table(rng, m)
    st8 = np.full((m, 8), np.nan)
    st8[:, :7] = st
    for mode in MODES:
        es, eq, ej, occ, win = run(ctx, codes, profile, off, lens, st, sq, mode)
        ctx.stage(codes)
        ctx.stage_codes2(codes2)
        ps, pt, pj, po, pw = ctx.expect_pair_joint_staged(sq, st8, mode, off, lens)
        assert rules.same_bits(ej, pj), where(ej, pj)
        assert rules.same_bits(es, pt) and rules.same_bits(eq, ps) and rules.same_bits(occ, po) and np.array_equal(win, pw)
        assert (ej > 0).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_identity_3_tables_of_ones_count_nucleotides(ctx, dtype):
    """every cell of R and S 1.0, ratio weights, no foreign code.  The letter chain: every weight is 1.0, rows of seven 0.5 give
    0.5 x the count of nucleotides.  The joint chain: the marginal of such a row is 3.5 and the weight 3.5^m (the table is
    3.5^m x 0.5 x the count, exact here); rows of dyadic cells that sum to 1.0 give the cell x the count"""
    from test_expect_profile_joint_cpu import DYADIC_ROW, nucleotide_counts
    rng = np.random.default_rng(57)
    m = 8
    codes, profile, off, lens = prules.stream(rng, length_ladder(rng, m, top=False), dtype)
    counts = nucleotide_counts(codes, off, lens, m).astype(np.float64)
    R, S = np.ones((m, 8)), np.ones((m, 7))
    inside = np.ones(len(profile), dtype=bool)
    inside[off + lens] = False                                          # the separator rows stay NaN
    profile[inside] = 0.5
    ej = run(ctx, codes, profile, off, lens, None, R, rules.RATIO)[2]
    assert np.array_equal(ej[:, 0, :, :, :7], 0.5 * counts[:, :, :, None] * np.ones(7)) and (ej[..., 7] == 0).all()
    ej = run(ctx, codes, profile, off, lens, S, R, rules.RATIO)[2]
    assert np.array_equal(ej[:, 0, :, :, :7], 3.5 ** m * 0.5 * counts[:, :, :, None] * np.ones(7))
    profile[inside] = DYADIC_ROW.astype(dtype)
    es, eq, ej, occ, win = run(ctx, codes, profile, off, lens, S, R, rules.RATIO)
    assert np.array_equal(ej[:, 0, :, :, :7], counts[:, :, :, None] * DYADIC_ROW) and np.array_equal(occ[:, 0], np.maximum(lens - m + 1, 0))


# ---- the _dev form and the refusals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dev_form_as_an_integrator_calls_it(ctx, dtype):
    """torch device tensors in and out, guard cells around every output; a subset record table; equal to _staged; the table
    alone, without the optional outputs"""
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
                torch.full((G + 4 * cells + G,), -7.0, dtype=torch.float64, device="cuda"),
                torch.full((G + n_rec * n_mo + G,), -7.0, dtype=torch.float64, device="cuda"), torch.full((G + n_rec + G,), -7, dtype=torch.int64, device="cuda"))

    for form in FORMS:
        a, b = tables(form, st, sq)
        for mode in MODES:
            want = run(ctx, codes, profile, off, lens, a, b, mode)
            d_st, d_sq, d_jt, d_occ, d_win = buffers()
            torch.cuda.synchronize()
            ctx.expect_profile_joint_dev(a, b, mode, d_codes.data_ptr(), d_prof.data_ptr(), code, codes.size, d_off.data_ptr(), d_len.data_ptr(), n_rec,
                                         d_st.data_ptr() + 8 * G, d_sq.data_ptr() + 8 * G, d_jt.data_ptr() + 8 * G, d_occ.data_ptr() + 8 * G,
                                         d_win.data_ptr() + 8 * G)
            ctx.synchronize()
            out = [x.cpu().numpy() for x in (d_st, d_sq, d_jt, d_occ, d_win)]
            for x in out:
                assert (x[:G] == -7).all() and (x[-G:] == -7).all()
            got = (out[0][G:-G].reshape(n_rec, n_mo, m, 8), out[1][G:-G].reshape(n_rec, n_mo, m, 8), out[2][G:-G].reshape(n_rec, n_mo, m, 4, 8),
                   out[3][G:-G].reshape(n_rec, n_mo), out[4][G:-G])
            assert rules.same(got, want)
            # the table alone, without the optional outputs
            _, _, d_jt, _, _ = buffers()
            torch.cuda.synchronize()
            ctx.expect_profile_joint_dev(a, b, mode, d_codes.data_ptr(), d_prof.data_ptr(), code, codes.size, d_off.data_ptr(), d_len.data_ptr(), n_rec,
                                         None, None, d_jt.data_ptr() + 8 * G)
            ctx.synchronize()
            x = d_jt.cpu().numpy()
            assert (x[:G] == -7).all() and (x[-G:] == -7).all() and rules.same_bits(x[G:-G].reshape(n_rec, n_mo, m, 4, 8), want[2])


def test_bad_arguments_launch_nothing(ctx):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(29)
    codes, profile, off, lens = prules.stream(rng, [50, 60, 70], np.float32)
    d_codes, d_prof = torch.from_numpy(codes).cuda(), torch.from_numpy(profile).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    d_st = torch.full((3, 2, 8, 8), -7.0, dtype=torch.float64, device="cuda")
    d_sq = torch.full((3, 2, 8, 8), -7.0, dtype=torch.float64, device="cuda")
    d_jt = torch.full((3, 2, 8, 4, 8), -7.0, dtype=torch.float64, device="cuda")
    d_occ = torch.full((3, 2), -7.0, dtype=torch.float64, device="cuda")
    d_win = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L, h, p = ctx._L, ctx._h, _lib._ptr
    S = np.ascontiguousarray(np.stack([prules.struct_table(rng, 8)] * 2))
    R = np.ascontiguousarray(np.stack([orules.table(rng, 8)] * 2))
    wide = np.ascontiguousarray(np.stack([prules.struct_table(rng, 65)] * 2))
    ptr = lambda t, shift=0: None if t is None else p(t.data_ptr() + shift)

    def dev(st=S, sq=R, n_mo=2, m=8, mode=1, c=d_codes, prof=d_prof, dt=_lib.PROFILE_F32, n_pos=codes.size, o=d_off, ln=d_len, n_rec=3, out=d_st,
            out_seq=d_sq, out_joint=d_jt, shift_prof=0, shift_codes=0):
        return L.pfmscan_expect_profile_joint_dev(h, p(st), p(sq), n_mo, m, mode, ptr(c, shift_codes), ptr(prof, shift_prof), dt, n_pos, ptr(o), ptr(ln),
                                                  n_rec, ptr(out), ptr(out_seq), ptr(out_joint), ptr(d_occ), ptr(d_win))
    assert dev(m=0) == _lib.E_BADSHAPE and dev(st=wide, m=65) == _lib.E_BADSHAPE
    assert dev(dt=_lib.PROFILE_NONE) == _lib.E_BADARG and dev(dt=3) == _lib.E_BADARG and dev(mode=2) == _lib.E_BADARG and dev(mode=-1) == _lib.E_BADARG
    assert dev(st=None, sq=None, out_seq=None, out_joint=None) == _lib.E_BADARG      # both tables NULL
    assert dev(sq=None, out_joint=None) == _lib.E_BADARG                              # exp_seq without seq_tables
    assert dev(sq=None, out_seq=None) == _lib.E_BADARG                                # the table without seq_tables
    assert dev(sq=None, out_seq=None, c=None) == _lib.E_BADARG
    assert dev(out=None, out_seq=None, out_joint=None) == _lib.E_BADARG               # all three outputs NULL
    assert dev(c=None) == _lib.E_BADARG and dev(prof=None) == _lib.E_BADARG
    assert dev(o=None) == _lib.E_BADARG and dev(ln=None) == _lib.E_BADARG
    assert dev(n_mo=-1) == _lib.E_BADARG and dev(n_rec=-1) == _lib.E_BADARG and dev(n_pos=-1) == _lib.E_BADARG
    assert dev(shift_prof=4) == _lib.E_BADSHAPE and dev(shift_codes=1) == _lib.E_BADSHAPE
    assert dev(n_pos=codes.size - 2) == _lib.E_BADARG                    # the last record runs past n_pos
    swapped = torch.from_numpy(off[[1, 0, 2]].copy()).cuda()
    longer = torch.from_numpy(lens + 1000).cuda()
    torch.cuda.synchronize()
    assert dev(o=swapped) == _lib.E_BADARG and dev(ln=longer) == _lib.E_BADARG
    assert dev(n_mo=0) == 0 and dev(n_rec=0) == 0                        # nothing to do: OK, nothing written
    ctx.synchronize()
    for t in (d_st, d_sq, d_jt, d_occ, d_win):
        assert (t.cpu().numpy() == -7).all()
    assert dev() == 0
    ctx.synchronize()
    want = rules.expected(profile, codes, off, lens, R, S, rules.POSTERIOR)
    assert rules.same((d_st.cpu().numpy(), d_sq.cpu().numpy(), d_jt.cpu().numpy(), d_occ.cpu().numpy(), d_win.cpu().numpy()), want)
    # the staged forms
    ctx.stage(codes, profile)
    out, outj = np.full((3, 2, 8, 8), -7.0), np.full((3, 2, 8, 4, 8), -7.0)
    staged = L.pfmscan_expect_profile_joint_staged
    assert staged(h, p(S), None, 2, 8, 1, p(off), p(lens), 3, p(out), None, p(outj), None, None) == _lib.E_BADARG    # the table without seq_tables
    assert staged(h, p(S), p(R), 2, 8, 1, p(off), p(lens), 3, None, None, None, None, None) == _lib.E_BADARG         # all three NULL
    assert staged(h, p(S), p(R), 2, 8, 2, p(off), p(lens), 3, p(out), None, p(outj), None, None) == _lib.E_BADARG    # mode
    acc = np.zeros((2, _lib.SITE_LIMBS, 32 * 8), dtype=np.uint64)
    merged = L.pfmscan_expect_profile_joint_merged_staged
    assert merged(h, p(S), p(R), 2, 8, 1, p(off), p(lens), 3, None, None, None, None, None, None, None, None) == _lib.E_BADARG
    assert merged(h, p(S), p(R), 2, 8, 1, p(off), p(lens), 3, None, None, p(acc), None, None, None, None, None) == _lib.E_BADARG   # no bad_joint
    assert merged(h, p(S), None, 2, 8, 1, p(off), p(lens), 3, None, None, p(acc), None, None, p(np.zeros((2, 2), dtype=np.int64)), None, None) == _lib.E_BADARG
    assert (out == -7).all() and (outj == -7).all() and not acc.any()
    with pytest.raises(ValueError):
        ctx.expect_profile_joint_staged(S, R, rules.POSTERIOR, off[[1, 0, 2]], lens)
    ctx.stage(None, profile)                                             # no codes staged
    with pytest.raises(ValueError):
        ctx.expect_profile_joint_staged(S, R, rules.POSTERIOR, off, lens)
