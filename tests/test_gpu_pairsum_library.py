"""Two-FASTA LIBRARIES with joint thresholds on the printed LogOdds.SeqStruct (pfmscan_library_hits_letters_sum_*,
k_library<.., uint8_t, true, SUM>): every pair in one pass of the library kernel, each against the per-pair call
(pfmscan_hits_pair_sum_host, which tests/test_gpu_pairsum.py checks against the oracle) -- several motif groups and passes,
finite and -inf thr_seq, a pair with a +inf cell, and the credit-table cache across plain and sum calls."""
import io

import numpy as np
import pytest

from pairsum_helpers import PairSumLibraryOracleEngine, lengths_for, printed_sum, streams, table

pytestmark = pytest.mark.gpu


def _per_pair(ctx, T, S, s1, s2, t1, t2, Ts):
    parts = []
    for k in range(len(T)):
        a, b = ctx.motif(T[k], None), ctx.motif(S[k], None)
        pos, sq, st = ctx.hits_pair_sum_host(a, b, s1.codes, s2.codes, t1, t2, float(Ts[k]))
        parts.append((pos, np.full(pos.size, k, dtype=np.int32), sq, st))
        a.close()
        b.close()
    pos, mo = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    order = np.lexsort((mo, pos))
    return pos[order], mo[order], np.concatenate([p[2] for p in parts])[order], np.concatenate([p[3] for p in parts])[order]


def _same(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (got[0].size, want[0].size)
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)) and np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64))


def _case(n, m, seed):
    from oracle import oracle
    rng = np.random.default_rng(seed)
    s1, s2 = streams(rng, lengths_for(rng, 8193, 9, m))
    T = np.stack([table(rng, m, 4) for _ in range(n)])
    S = np.stack([table(rng, m, 7, dyadic=(k % 3 == 0)) for k in range(n)])
    S[1, m // 2, 2], T[2, 0, 1] = -np.inf, -np.inf                     # -inf cells on either side
    Ts = np.empty(n)
    for k in range(n):                                                  # per pair: a T that about 1 % of the windows pass, ON a printed sum
        sq, st = oracle.stream_seq(s1.codes, T[k]), oracle.stream_letters_f64(s2.codes, S[k])
        p = printed_sum(sq, st)
        Ts[k] = np.sort(p[np.isfinite(p)])[-80]
    return s1, s2, T, S, Ts


@pytest.mark.parametrize("m", [8, 12, 17])
@pytest.mark.parametrize("n", [3, 13, 25])
def test_library_equals_the_per_pair_calls(ctx, n, m):
    from rnascan_amd import _lib
    s1, s2, T, S, Ts = _case(n, m, 900 + 31 * n + m)
    lib = ctx.library(T, struct_letters=S)
    for t1, t2 in ((-np.inf, -np.inf), (-1.0, -np.inf), (-np.inf, -2.0), (0.5, -1.0)):
        eff = _lib.library_letters_sum_thresholds(T, S, t1, Ts)
        assert np.isfinite(eff).all() and (eff >= t1).all()
        got = ctx.library_hits_letters_sum_host(lib, s1.codes, s2.codes, t1, t2, Ts)
        want = _per_pair(ctx, T, S, s1, s2, t1, t2, Ts)
        _same(got, want)
        plain = ctx.library_hits_letters_host(lib, s1.codes, s2.codes, t1, t2) if np.isfinite(t1) else None
        assert got[0].size > 0 and (plain is None or got[0].size < plain[0].size), "the case must hold hits and windows only the joint threshold drops"
    # thr_sum = -inf for every pair: exactly the plain call
    _same(ctx.library_hits_letters_sum_host(lib, s1.codes, s2.codes, 0.5, -1.0, -np.inf), ctx.library_hits_letters_host(lib, s1.codes, s2.codes, 0.5, -1.0))
    with pytest.raises(ValueError):
        ctx.library_hits_letters_sum_host(lib, s1.codes, s2.codes, 0.5, -1.0, np.nan)
    lib.close()


def test_a_pair_with_a_plus_inf_cell(ctx):
    """no bound on that pair's structure score: thr_eff stays thr_seq -- the same hits at a finite thr_seq, a closed route at -inf"""
    from rnascan_amd import _lib
    s1, s2, T, S, Ts = _case(5, 12, 77)
    S[3, 4, 1] = np.inf
    lib = ctx.library(T, struct_letters=S)
    eff = _lib.library_letters_sum_thresholds(T, S, -50.0, Ts)
    assert eff[3] == -50.0 and (eff[[0, 1, 2, 4]] > -50.0).all()
    _same(ctx.library_hits_letters_sum_host(lib, s1.codes, s2.codes, -0.5, -np.inf, Ts), _per_pair(ctx, T, S, s1, s2, -0.5, -np.inf, Ts))
    closed = _lib.library_letters_sum_thresholds(T, S, -np.inf, Ts)
    assert np.isneginf(closed[3]) and np.isfinite(closed[[0, 1, 2, 4]]).all()
    with pytest.raises(ValueError):
        ctx.library_hits_letters_sum_host(lib, s1.codes, s2.codes, -np.inf, -np.inf, Ts)
    lib.close()


def test_credit_tables_are_rebuilt_between_plain_and_sum_calls(ctx):
    """the device tables are keyed on thr_eff and T as well: credits tightened for one call must not drop the hits of the next"""
    s1, s2, T, S, Ts = _case(13, 12, 78)
    lib = ctx.library(T, struct_letters=S)
    plain = ctx.library_hits_letters_host(lib, s1.codes, s2.codes, -1.0, -1.0)
    first = ctx.library_hits_letters_sum_host(lib, s1.codes, s2.codes, -1.0, -1.0, Ts)
    other = ctx.library_hits_letters_sum_host(lib, s1.codes, s2.codes, -1.0, -1.0, Ts - 2.0)
    again = ctx.library_hits_letters_host(lib, s1.codes, s2.codes, -1.0, -1.0)
    repeat = ctx.library_hits_letters_sum_host(lib, s1.codes, s2.codes, -1.0, -1.0, Ts)
    _same(again, plain)
    _same(repeat, first)
    _same(first, _per_pair(ctx, T, S, s1, s2, -1.0, -1.0, Ts))
    _same(other, _per_pair(ctx, T, S, s1, s2, -1.0, -1.0, Ts - 2.0))
    assert first[0].size < other[0].size < plain[0].size
    lib.close()


def test_dev_form_on_a_callers_stream(ctx):
    import torch
    s1, s2, T, S, Ts = _case(13, 8, 79)
    lib = ctx.library(T, struct_letters=S)
    want = ctx.library_hits_letters_sum_host(lib, s1.codes, s2.codes, -np.inf, -1.0, Ts)
    dev = torch.device("cuda:%d" % ctx.device)
    d1, d2 = torch.from_numpy(s1.codes).to(dev), torch.from_numpy(s2.codes).to(dev)
    cap = int(want[0].size) + 9
    hp = torch.full((cap,), -1, dtype=torch.int64, device=dev)
    hm = torch.zeros(cap, dtype=torch.int32, device=dev)
    hq = torch.zeros(cap, dtype=torch.float32, device=dev)
    ht = torch.zeros(cap, dtype=torch.float64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ctx.library_hits_letters_sum_dev(lib, d1.data_ptr(), d2.data_ptr(), s1.n_pos, -np.inf, -1.0, Ts, cap, hp.data_ptr(), hm.data_ptr(),
                                     hq.data_ptr(), ht.data_ptr(), cnt.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    k = int(cnt.item())
    assert k == want[0].size
    pos, mo = hp[:k].cpu().numpy(), hm[:k].cpu().numpy()
    order = np.lexsort((mo, pos))
    _same((pos[order], mo[order], hq[:k].cpu().numpy()[order], ht[:k].cpu().numpy()[order]), want)
    lib.close()


def test_cli_library_takes_the_library_route(tmp_path):
    """`-p seq_lib -q struct_lib seqs.fa structs.fa --min-seqstruct T`: width groups of several pairs are one library call each,
    at a finite -m and at -m ' -inf' -- the oracle-backed engine's bytes"""
    from rnascan_amd import cli, scanner
    from test_gpu_pairsum import _fasta_pair, _sums
    from test_scanner_cpu import _write_multi_pfm
    rng = np.random.default_rng(54)
    seq_m, st_m = [], []
    for k in range(7):
        w = [8, 8, 12, 8, 12, 12, 8][k]
        seq_m.append(("RBP%02d" % k, list("ACGU"), rng.dirichlet(np.full(4, 0.5), size=w)))
        st_m.append(("RBP%02d" % k, list("EHTBLRM"), rng.dirichlet(np.full(7, 0.5), size=w)))
    _write_multi_pfm(str(tmp_path / "sq.pfm"), seq_m)
    _write_multi_pfm(str(tmp_path / "st.pfm"), st_m)
    _fasta_pair(tmp_path / "s.fa", tmp_path / "t.fa", [int(x) for x in rng.integers(0, 500, size=20)], rng)
    argv = ["-p", str(tmp_path / "sq.pfm"), "-q", str(tmp_path / "st.pfm"), "-u", "-C", "0.01", str(tmp_path / "s.fa"), str(tmp_path / "t.fa")]

    def run(args, eng):
        out = io.StringIO()
        cli.main(args, engine=eng, out=out)
        return out.getvalue()

    engine = scanner.HipEngine(0)
    calls = []
    inner = engine.library_hits_letters_sum
    engine.library_hits_letters_sum = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    try:
        for minscore in ("-1", " -inf"):
            sums = _sums(run(["-m", minscore] + argv, engine))
            assert sums.size > 10
            T = float(np.sort(sums)[-max(5, sums.size // 50)])
            del calls[:]
            got = run(["-m", minscore, "--min-seqstruct", repr(T)] + argv, engine)
            assert len(calls) == 2, "one library call per width group"
            assert got == run(["-m", minscore, "--min-seqstruct", repr(T)] + argv, PairSumLibraryOracleEngine())
            assert 1 < got.count("\n") < sums.size + 1
    finally:
        engine.close()
