"""k_exp_merge (csrc/pfmscan_expect_merge.hip) and the *_merged_staged forms on the GPU against the integers of
tests/expect_merge_rules.py, and the three commands' ``--merge device`` against ``--merge host`` byte for byte.  Limbs are
compared exactly; there is no tolerance in the contract."""
import os

import numpy as np
import pytest

import expect_merge_rules as mrules
import occupancy_profile_rules as prules
import occupancy_rules as orules
import pair_rules
import test_expect_cpu as ecpu
import test_expect_profile_cpu as pcpu
import test_pair_cpu as qcpu
from test_expect_merge_cpu import draw
from test_occupancy_profile_cpu import FILE_ORDER, STRUCT, make_inputs, write_profile

pytestmark = pytest.mark.gpu

LIMBS = mrules.LIMBS
SHAPES = [(1, 1, 1), (2, 3, 12), (33, 1, 12), (257, 3, 64), (5000, 3, 2)]
DBL_MAX = float(np.finfo(np.float64).max)


def crafted(shape, seed):
    """bit patterns over the whole exponent field, zeros of both signs, the edges, and one cell whose sum passes DBL_MAX"""
    n_rec, n_mo, m = shape
    rng = np.random.default_rng(seed)
    exp = draw(rng, (n_rec, n_mo, m, 8))
    # the top of the exponent field is record 0's: 2^13 later records of it would pass DBL_MAX in nearly every cell
    bits = exp[1:].view(np.uint64)
    bits[(bits >> np.uint64(52)) > 2032] -= np.uint64(14 << 52)
    flat = exp.reshape(-1)
    kinds = rng.integers(0, 12, size=flat.size)
    flat[kinds == 0] = 0.0
    flat[kinds == 1] = -0.0
    flat[kinds == 2] = draw(rng, int((kinds == 2).sum()), 0, 0)           # subnormals
    flat[kinds == 3] = 2.0 ** rng.integers(-1074, 1010, size=int((kinds == 3).sum())).astype(np.float64)
    special = [5e-324, DBL_MAX, 2.0 ** -1022, 2.0 ** 1023, 1.0]
    flat[:len(special)] = special[:flat.size]
    exp[:, n_mo - 1, m - 1, 6] = DBL_MAX if n_rec > 1 else 1.5            # two of them are beyond DBL_MAX
    return exp


def merge_dev(ctx, exp, zero_first=True, d_acc=None, d_bad=None):
    """-> (d_acc, d_bad) torch tensors after the call"""
    import torch
    n_rec, n_mo, m = exp.shape[:3]
    d_exp = torch.from_numpy(np.ascontiguousarray(exp)).cuda()
    if d_acc is None:
        d_acc = torch.full((n_mo, LIMBS, m * 8), 12345, dtype=torch.int64, device="cuda")
        d_bad = torch.full((n_mo, 2), 777, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.expect_merge_dev(d_exp.data_ptr(), n_rec, n_mo, m, zero_first, d_acc.data_ptr(), d_bad.data_ptr())
    ctx.synchronize()
    return d_acc, d_bad


def home(d_acc):
    return d_acc.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def cases():
    """every shape's tensor and its integers, once"""
    out = {}
    for i, shape in enumerate(SHAPES):
        exp = crafted(shape, 40 + i)
        out[shape] = (exp, mrules.merge_ints(exp))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_against_the_integers(ctx, cases, shape):
    from rnascan_amd import _lib
    exp, A = cases[shape]
    d_acc, d_bad = merge_dev(ctx, exp)
    raw = home(d_acc)
    assert (raw < 1 << 63).all()
    assert (mrules.normalise(raw) == mrules.limbs_of(A)).all()
    assert (d_bad.cpu().numpy() == -1).all()
    got = _lib.site_acc_round(raw)
    want = mrules.rounded(A)
    assert got.tobytes() == want.tobytes()
    n_mo, m = shape[1:]
    big = (n_mo - 1, (m - 1) * 8 + 6)
    assert np.isposinf(got[big]) == (shape[0] > 1)
    finite = np.isfinite(want)                                            # math.fsum raises where the sum overflows
    assert finite.mean() > 0.9 and finite[big] == (shape[0] == 1)
    summed = mrules.fsum_cells(np.where(finite.reshape((1, n_mo, m, 8)), exp, 0.0))
    assert got[finite].tobytes() == summed[finite].tobytes()


def test_order_and_batching_do_not_change_a_limb(ctx, cases):
    shape = (257, 3, 64)
    exp, A = cases[shape]
    want = mrules.limbs_of(A)
    rng = np.random.default_rng(7)
    d_acc, _ = merge_dev(ctx, exp[rng.permutation(shape[0])])
    assert (mrules.normalise(home(d_acc)) == want).all()
    d_acc, d_bad = merge_dev(ctx, exp[:100], True)
    merge_dev(ctx, exp[100:101], False, d_acc, d_bad)
    merge_dev(ctx, exp[101:], False, d_acc, d_bad)
    assert (mrules.normalise(home(d_acc)) == want).all() and (d_bad.cpu().numpy() == -1).all()


def test_rejected_cells_add_nothing_and_name_their_record(ctx, cases):
    shape = (257, 3, 64)
    exp = cases[shape][0].copy()
    exp[:, 2, 63, 6] = 1.0
    clean = exp.copy()
    plant = [(200, 0, 5, 3, np.nan), (70, 0, 63, 7, np.inf), (131, 1, 0, 0, -1.0), (30, 1, 9, 2, -np.inf), (256, 1, 9, 2, -2.5)]
    for r, k, row, c, v in plant:
        exp[r, k, row, c] = v
        clean[r, k, row, c] = 0.0
    d_acc, d_bad = merge_dev(ctx, exp)
    want_bad = mrules.bad(exp)
    assert want_bad.tolist() == [[70, -1], [30, 30], [-1, -1]]
    assert (d_bad.cpu().numpy() == want_bad).all()
    # the planted values have added nothing: the accumulators are those of the tensor with zeros in their places
    assert (mrules.normalise(home(d_acc)) == mrules.limbs_of(mrules.merge_ints(clean))).all()
    # added to earlier verdicts, the smaller index stays
    import torch
    before = np.array([[10, -1], [100, 3], [5, 5]], dtype=np.int64)
    d_bad = torch.from_numpy(before.copy()).cuda()
    d_acc = torch.zeros((3, LIMBS, 64 * 8), dtype=torch.int64, device="cuda")
    merge_dev(ctx, exp, False, d_acc, d_bad)
    assert (d_bad.cpu().numpy() == mrules.bad(exp, before)).all() and mrules.bad(exp, before).tolist() == [[10, -1], [30, 3], [5, 5]]


def test_bad_arguments_and_empty_calls(ctx):
    import torch
    from rnascan_amd import _lib
    d_exp = torch.ones((2, 2, 3, 8), dtype=torch.float64, device="cuda")
    d_acc = torch.full((2, LIMBS, 24), 9, dtype=torch.int64, device="cuda")
    d_bad = torch.full((2, 2), 9, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L, h = ctx._L, ctx._h
    call = lambda e=d_exp.data_ptr(), n_rec=2, n_mo=2, m=3, z=1, a=d_acc.data_ptr(), b=d_bad.data_ptr(): L.pfmscan_expect_merge_dev(h, e, n_rec, n_mo, m, z, a, b)
    assert call(m=0) == _lib.E_BADSHAPE and call(m=65) == _lib.E_BADSHAPE
    assert call(e=None) == _lib.E_BADARG and call(a=None) == _lib.E_BADARG and call(b=None) == _lib.E_BADARG and call(n_rec=-1) == _lib.E_BADARG
    ctx.synchronize()
    assert (d_acc.cpu().numpy() == 9).all() and (d_bad.cpu().numpy() == 9).all()
    assert call(n_rec=0, z=0) == 0
    ctx.synchronize()
    assert (d_acc.cpu().numpy() == 9).all()
    assert call(n_rec=0) == 0                                            # nothing to add: zeroed as asked
    ctx.synchronize()
    assert (d_acc.cpu().numpy() == 0).all() and (d_bad.cpu().numpy() == -1).all()
    assert call(z=0) == 0
    ctx.synchronize()
    assert (home(d_acc) == mrules.limbs_of(mrules.merge_ints(np.ones((2, 2, 3, 8))))).all()


# ---- the staged forms ------------------------------------------------------------------------------------------------
def stream_lengths(rng, m):
    return [int(x) for x in rng.integers(0, 201, size=37)] + [max(m - 1, 0), 0, 200]


def fsum_over_records(exp):
    from rnascan_amd import expect
    n_mo = exp.shape[1]
    return np.stack([expect.fsum_records([exp[:, k]]) for k in range(n_mo)])


def check_staged(pairs_of_results, occ_pair, win_pair):
    from rnascan_amd import _lib
    for acc, bad, exp in pairs_of_results:
        assert (bad == -1).all()
        got = _lib.site_acc_round(acc).reshape(exp.shape[1:])
        assert got.tobytes() == fsum_over_records(exp).tobytes()
    assert occ_pair[0].tobytes() == occ_pair[1].tobytes() and np.array_equal(win_pair[0], win_pair[1])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("m", [1, 12])
def test_expect_merged_staged(ctx, m, mode):
    from rnascan_amd import expect
    rng = np.random.default_rng(60 + m + mode)
    codes, off, lens = orules.stream(rng, stream_lengths(rng, m), 4, foreign=0.01)
    R = np.stack([orules.table(rng, m, 4, 0.5, 2.0) for _ in range(3)])
    R[2, 0, :4] = 0.0                                                     # motif 2: every occupancy is 0
    ctx.stage(codes)
    exp, occ, win = ctx.expect_staged(R, 4, mode, off, lens)
    assert (occ[:, 2] == 0).all() and (lens < m).any()
    acc = expect.new_acc(3, m)
    bad, occ2, win2 = ctx.expect_merged_staged(R, 4, mode, off, lens, acc)
    check_staged([(acc, bad, exp)], (occ, occ2), (win, win2))
    # two batches added into one accumulator
    two = expect.new_acc(3, m)
    cut = 17
    for a, b in ((0, cut), (cut, len(off))):
        o, n = off[a:b] - off[a], lens[a:b]
        ctx.stage(codes[off[a]:off[b - 1] + lens[b - 1] + 1])
        ctx.expect_merged_staged(R, 4, mode, o, n, two)
    assert (two == acc).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("m", [1, 12])
def test_expect_profile_merged_staged(ctx, m, mode, dtype):
    from rnascan_amd import expect
    rng = np.random.default_rng(70 + m + mode)
    codes, profile, off, lens = prules.stream(rng, stream_lengths(rng, m), dtype, foreign=0.01)
    st = np.stack([prules.struct_table(rng, m, 0.5, 2.0) for _ in range(3)])
    sq = np.stack([orules.table(rng, m, 4, 0.5, 2.0) for _ in range(3)])
    sq[2, 0, :4] = 0.0
    ctx.stage(codes, profile)
    es, eq, occ, win = ctx.expect_profile_staged(st, sq, mode, off, lens)
    a_st, a_sq = expect.new_acc(3, m), expect.new_acc(3, m)
    b_st, b_sq, occ2, win2 = ctx.expect_profile_merged_staged(st, sq, mode, off, lens, a_st, a_sq)
    check_staged([(a_st, b_st, es), (a_sq, b_sq, eq)], (occ, occ2), (win, win2))
    # structure only: no sequence accumulator
    es, _, occ, win = ctx.expect_profile_staged(st, None, mode, off, lens)
    one = expect.new_acc(3, m)
    b_st, b_sq, occ2, win2 = ctx.expect_profile_merged_staged(st, None, mode, off, lens, one)
    assert b_sq is None
    check_staged([(one, b_st, es)], (occ, occ2), (win, win2))
    ctx.expect_profile_merged_staged(st, None, mode, off, lens, one)      # the same records again: twice the integers
    assert (mrules.normalise(one) == mrules.limbs_of(2 * mrules.merge_ints(es))).all()
    with pytest.raises(ValueError):
        ctx.expect_profile_merged_staged(st, None, mode, off, lens, one, a_sq)      # acc_seq needs seq_tables


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("m", [1, 12])
def test_expect_pair_merged_staged(ctx, m, mode):
    from rnascan_amd import expect
    rng = np.random.default_rng(80 + m + mode)
    codes, codes2, off, lens = pair_rules.streams(rng, stream_lengths(rng, m), foreign_seq=0.01, foreign_struct=0.01, case=True)
    R = np.stack([pair_rules.table(rng, m, 4, 0.6, 1.7) for _ in range(3)])
    S = np.stack([pair_rules.table(rng, m, 7, 0.6, 1.7) for _ in range(3)])
    S[2, 0, :7] = 0.0
    ctx.stage(codes)
    ctx.stage_codes2(codes2)
    eq, es, occ, win = ctx.expect_pair_staged(R, S, mode, off, lens)
    a_sq, a_st = expect.new_acc(3, m), expect.new_acc(3, m)
    b_sq, b_st, occ2, win2 = ctx.expect_pair_merged_staged(R, S, mode, off, lens, a_sq, a_st)
    check_staged([(a_sq, b_sq, eq), (a_st, b_st, es)], (occ, occ2), (win, win2))
    only = expect.new_acc(3, m)
    b_sq, b_st, _, _ = ctx.expect_pair_merged_staged(R, S, mode, off, lens, None, only)
    assert b_sq is None and (only == a_st).all() and (b_st == -1).all()
    with pytest.raises(ValueError):
        ctx.expect_pair_merged_staged(R, S, mode, off, lens, None, None)


def test_staged_form_reports_a_nonfinite_cell(ctx):
    from rnascan_amd import expect
    rng = np.random.default_rng(90)
    codes, off, lens = orules.stream(rng, [30, 5, 40, 50], 4)
    codes[off[2]:off[2] + 40] = 1
    codes[off[0]:off[0] + 30] = 2
    codes[off[3]:off[3] + 50] = 1
    R = np.stack([orules.table(rng, 6, 4, 0.5, 2.0) for _ in range(2)])
    R[1, 3, 1] = np.inf                                                   # letter 1 under column 3: records 2 and 3
    ctx.stage(codes)
    acc = expect.new_acc(2, 6)
    bad, occ, _ = ctx.expect_merged_staged(R, 4, 0, off, lens, acc)
    exp, occ_h, _ = ctx.expect_staged(R, 4, 0, off, lens)
    assert bad.tolist() == mrules.bad(exp).tolist() == [[-1, -1], [2, -1]] and occ.tobytes() == occ_h.tobytes()


# ---- the commands ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


def device_equals_host(run, outputs, engine, argv, tmp_path, inputs):
    assert run(engine, argv + ["--merge", "host", "-o", str(tmp_path / "host")] + inputs) == 0
    want = outputs(tmp_path / "host")
    for extra in (["--merge", "device", "--batch-records", "1"], ["--merge", "device", "--batch-records", "3"], ["--merge", "device", "--batch-records", "4096"], []):
        assert run(engine, argv + extra + ["-o", str(tmp_path / "dev")] + inputs) == 0
        assert outputs(tmp_path / "dev") == want, extra
    return want


def test_expect_command_device_equals_host(engine, tmp_path):
    fa = tmp_path / "s.fa"
    fa.write_text(ecpu.FASTA)
    pfm = ecpu.write_pfm(tmp_path / "lib.pfm", "ACGU", (6, 4, 6), seed=5)
    for weight in ("posterior", "ratio"):
        device_equals_host(ecpu.run_command, ecpu.outputs, engine, ["-p", pfm, "-C", "0.1", "--all-motifs", "--iterations", "2", "--weight", weight], tmp_path, [str(fa)])


def test_expect_pair_command_device_equals_host(engine, tmp_path):
    fa, sfa = qcpu.write_inputs(tmp_path)
    seq = ecpu.write_pfm(tmp_path / "seq.pfm", "ACGU", (6, 4), seed=3)
    st = ecpu.write_pfm(tmp_path / "st.pfm", STRUCT, (6, 4), seed=4)
    device_equals_host(qcpu.run_expect, qcpu.outputs, engine,
                       ["-p", seq, "-q", st, "-u", "-C", "0.02", "--struct-format", "letters", "--all-motifs", "--iterations", "2"], tmp_path, [fa, sfa])


@pytest.mark.parametrize("form", ["struct", "joint", "seq"])
def test_expect_profile_command_device_equals_host(engine, tmp_path, form):
    other = "EHTBLRM"
    fa, d, st, data, order = make_inputs(tmp_path)
    _, mixed, _, _, _ = make_inputs(tmp_path, orders=[FILE_ORDER, other, other, FILE_ORDER, other, FILE_ORDER], name="mixed")
    seq = pcpu.write_pfm(tmp_path / "seq.pfm", "ACGU", (6, 4), seed=2, ids=["A", "B"])
    stp = pcpu.write_pfm(tmp_path / "st.pfm", STRUCT, (6, 4), seed=3, ids=["A", "B"])
    opts = (["-p", seq] if form != "struct" else []) + (["-q", stp] if form != "seq" else [])
    outputs = lambda prefix: pcpu.outputs(prefix, form != "struct")
    inputs = lambda source, fasta: [source] if form == "struct" else [fasta, source]
    device_equals_host(pcpu.run_command, outputs, engine, opts + ["-u", "-C", "0.01", "--all-motifs", "--iterations", "2"], tmp_path, inputs(st, fa))
    # two text files' column orders in one directory: every run is mapped to the letters before the runs are added
    device_equals_host(pcpu.run_command, outputs, engine, opts + ["-u", "-C", "0.01", "--all-motifs"], tmp_path, inputs(mixed, str(tmp_path / "mixed.fa")))


def test_a_negative_cell_and_a_zero_background(engine, tmp_path, capsys):
    fa, d, st, data, order = make_inputs(tmp_path)
    rows = data["r3"][1].copy()
    rows[:, 2] = -0.05
    write_profile(d, "r3", rows)
    stp = pcpu.write_pfm(tmp_path / "st.pfm", STRUCT, (6,), seed=3)
    base = ["-q", stp, "-u", "-C", "0.01"]
    assert pcpu.run_command(engine, base + ["--merge", "host", "-o", str(tmp_path / "host"), d]) == 0
    capsys.readouterr()
    assert pcpu.run_command(engine, base + ["-o", str(tmp_path / "auto"), d]) == 0
    err = capsys.readouterr().err
    assert pcpu.outputs(tmp_path / "auto", False) == pcpu.outputs(tmp_path / "host", False)
    assert "record r3" in err and "negative" in err and "on the host" in err
    assert pcpu.run_command(engine, base + ["--merge", "device", "-o", str(tmp_path / "dev"), d]) == 1
    err = capsys.readouterr().err
    assert "record r3" in err and "negative" in err and not os.path.exists(str(tmp_path / "dev") + ".summary.txt")
    # a background of 0 under a used letter: both routes end with the same message
    sfa = tmp_path / "s.fa"
    sfa.write_text(ecpu.FASTA)
    seq = ecpu.write_pfm(tmp_path / "seq.pfm", "ACGU", (6,))
    bg = tmp_path / "bg.txt"
    bg.write_text("{'A': 0.0, 'C': 0.3, 'G': 0.3, 'U': 0.4}")
    said = []
    for weight in ("posterior", "ratio"):
        for merge in ("host", "device"):
            assert ecpu.run_command(engine, ["-p", seq, "-C", "0.01", "-b", str(bg), "--weight", weight, "--merge", merge, "-o", str(tmp_path / "bad"), str(sfa)]) == 1
            said.append(capsys.readouterr().err)
    assert said[0] == said[1] and said[2] == said[3] and "record r1" in said[0] and "Motif seq" in said[2]
