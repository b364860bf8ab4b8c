"""Combined hits with the joint threshold on LogOdds.SeqStruct, decided on the device (pfmscan_hits_sum_*).

The oracle for every test:  want_sum = float64(np.round(float32 seq, 3)) + struct  with the oracle's two scores -- the
printed column -- and the expected hits are the plain combined hits whose want_sum exceeds T (strict; NaN never passes).
Hit SETS are the oracle's exactly on every kernel that decides one (k_profile, k_profile_fixed, k_struct_at, k_wide), also
with T planted ON a window's sum or one ulp beside it, where the kernel's fast structure score would decide otherwise:
there the window is re-scored in the reference's rounded order (rnascan_amd/csrc/pfmscan_exact.hpp)."""
import ctypes
import io

import numpy as np
import pytest

from conftest import assert_f32_bits_equal
from precision_rules import assert_struct_tight
from test_gpu_dev_streams import DEV, HitsDev, _behind_delay, _ptr, _timed_plain_run, delay    # noqa: F401 (delay: a fixture)
from test_gpu_parity import rand_stream, rand_struct_pssm, rand_table

pytestmark = pytest.mark.gpu


def want_sum_of(want_seq, want_st):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.round(want_seq, 3).astype(np.float64) + want_st


def want_hits(oracle, want_seq, want_st, thr_seq, thr_struct, T):
    pos = oracle.stream_hits(want_seq, want_st, thr_seq, thr_struct)
    with np.errstate(invalid="ignore"):
        return pos[want_sum_of(want_seq, want_st)[pos] > T]


def check(got, want_pos, want_seq, profile, P, what):
    pos, sq, st = got
    assert np.array_equal(pos, want_pos), (what, pos.size, want_pos.size)
    assert_f32_bits_equal(sq, want_seq[want_pos])                        # the reported sequence score, bit for bit
    assert_struct_tight(st, profile, P, positions=want_pos)              # the structure score within its rounding-error bound


def spoil_rows(rng, s):
    """a few profile rows holding NaN / +inf (the per-row nan_to_num cases); returns the stream"""
    rows = rng.choice(s.profile.shape[0], size=6, replace=False)
    s.profile[rows[:3], rng.integers(0, 7, size=3)] = np.nan
    s.profile[rows[3:], rng.integers(0, 7, size=3)] = np.inf
    return s


def struct_pssm(rng, m, cells):
    """a structure PSSM, all finite or with two -inf cells and a NaN cell (the per-row nan_to_num form).  Few enough that a
    good share of the windows keeps a finite score at every width: a window covers every row of the PSSM."""
    P = rand_struct_pssm(rng, m)
    if cells == "inf":
        at = rng.choice(m * 7, size=3, replace=False)
        P.reshape(-1)[at[:2]] = -np.inf
        P.reshape(-1)[at[2]] = np.nan
    return P


def quantiles(values, qs):
    v = values[np.isfinite(values) & (np.abs(values) < 1e300)]
    assert v.size > 50
    return [float(np.quantile(v, q)) for q in qs]


# ---- hit sets on every kernel ----------------------------------------------------------------------------------------
# 7: generic k_profile (< 9 rows); 12, 18: k_profile_fixed; 24: generic; 64: the widest tuned width; 100: k_profile beyond 64;
# 200: k_wide
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m", [7, 12, 18, 24, 64, 100, 200])
def test_hit_sets_equal_the_oracle(oracle, monkeypatch, m, dtype):
    from rnascan_amd import _lib
    rng = np.random.default_rng(3000 + m + (1 if dtype == np.float64 else 0))
    s = spoil_rows(rng, rand_stream(rng, 13, 200, 2500, dtype=dtype))
    T_tab = rand_table(rng, m)
    want_seq = oracle.stream_seq(s.codes, T_tab)
    cases = []
    for cells in ("finite", "inf"):
        P = struct_pssm(rng, m, cells)
        want_st = oracle.stream_struct(s.profile, P)
        cases.append((cells, P, want_st))
    n_checked = 0
    for two_phase in (0, 1):
        monkeypatch.setenv("PFMSCAN_TWO_PHASE", str(two_phase))
        with _lib.Context(0) as c:
            c.stage(s.codes, s.profile)
            for cells, P, want_st in cases:
                motif = c.motif(T_tab, P)
                for thr_kind in ("-inf", "q0.9"):
                    if thr_kind == "-inf":
                        if two_phase:
                            continue                       # an infinite thr_seq never takes two passes: covered at two_phase = 0
                        thr_seq = thr_st = -np.inf
                    else:
                        thr_seq = quantiles(want_seq.astype(np.float64), [0.9])[0]
                        thr_st = quantiles(want_st, [0.1])[0]
                    plain = oracle.stream_hits(want_seq, want_st, thr_seq, thr_st)
                    for T in quantiles(want_sum_of(want_seq, want_st)[plain], [0.1, 0.5, 0.9]):
                        want_pos = want_hits(oracle, want_seq, want_st, thr_seq, thr_st, T)
                        assert 0 < want_pos.size < plain.size
                        check(c.hits_sum_staged(motif, thr_seq, thr_st, T), want_pos, want_seq, s.profile, P,
                              (m, cells, thr_kind, two_phase, T))
                        n_checked += 1
                motif.close()
    assert n_checked == 2 * 3 * 3


# ---- thresholds planted ON the sum and one ulp beside it --------------------------------------------------------------
def _planted(oracle, c, s, T_tab, P, thr_seq, thr_st, rng, need_differ):
    from test_seqstruct_cpu import round3
    motif = c.motif(T_tab, P)
    want_seq, want_st = oracle.stream_seq(s.codes, T_tab), oracle.stream_struct(s.profile, P)
    want_sum = want_sum_of(want_seq, want_st)
    _, fast_st = c.scan_host(motif, s.codes, s.profile)
    with np.errstate(invalid="ignore", over="ignore"):
        fast_sum = round3(want_seq).astype(np.float64) + fast_st             # what a compare of the fast score would see
    eligible = np.zeros(want_sum.size, bool)
    eligible[oracle.stream_hits(want_seq, want_st, thr_seq, thr_st)] = True
    eligible &= np.isfinite(want_sum) & (np.abs(want_sum) < 1e300)
    differ = np.flatnonzero(eligible & (fast_sum != want_sum))
    assert differ.size >= need_differ, "the fast sum equals the oracle's everywhere: this test would prove nothing"
    picks = rng.choice(differ, size=min(4, differ.size), replace=False).tolist()
    if len(picks) < 4:
        rest = np.setdiff1d(np.flatnonzero(eligible), np.array(picks, dtype=np.int64))
        picks += rng.choice(rest, size=4 - len(picks), replace=False).tolist()
    for p in picks:
        on = float(want_sum[p])
        for T in (on, float(np.nextafter(on, -np.inf)), float(np.nextafter(on, np.inf))):
            pos, sq, st = c.hits_sum_host(motif, s.codes, s.profile, thr_seq, thr_st, T)
            want_pos = want_hits(oracle, want_seq, want_st, thr_seq, thr_st, T)
            assert np.array_equal(pos, want_pos), (p, T, pos.size, want_pos.size)
            at = np.flatnonzero(pos == p)
            if T < on:                                     # one ulp below: p is a hit, reported with the re-scored value
                assert at.size == 1 and st[at[0]] == want_st[p]
            else:                                          # ON the sum (strict >) or above it: p is out
                assert at.size == 0
    motif.close()


@pytest.mark.parametrize("cells", ["finite", "inf"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("path", ["fused-12", "fused-24", "struct_at-12", "wide-200"])
def test_thresholds_on_and_beside_the_sum(oracle, monkeypatch, path, dtype, cells):
    from rnascan_amd import _lib
    kind, m = path.split("-")
    m = int(m)
    monkeypatch.setenv("PFMSCAN_TWO_PHASE", "1" if kind == "struct_at" else "0")
    rng = np.random.default_rng(4100 + m + (1 if dtype == np.float64 else 0) + (2 if cells == "inf" else 0) + (4 if kind == "struct_at" else 0))
    s = rand_stream(rng, 12 if m < 100 else 6, 200 if m < 100 else 600, 2500 if m < 100 else 1500, dtype=dtype)
    T_tab = rand_table(rng, m)
    P = struct_pssm(rng, m, cells)
    want_seq = oracle.stream_seq(s.codes, T_tab)
    if kind == "struct_at":                                # selective: the letters pass + k_struct_at
        thr_seq, thr_st = quantiles(want_seq.astype(np.float64), [0.985])[0], -np.inf
    elif kind == "fused":
        thr_seq, thr_st = quantiles(want_seq.astype(np.float64), [0.5])[0], -np.inf
    else:
        thr_seq = thr_st = -np.inf
    # (with float32 rows or -inf cells the two orders agree almost everywhere, as for the structure threshold)
    need = 4 if (cells == "finite" and dtype == np.float64) else 0
    with _lib.Context(0) as c:
        _planted(oracle, c, s, T_tab, P, thr_seq, thr_st, rng, need)


# ---- the rounding on the device ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [12, 24])
def test_rounding_on_the_device(ctx, oracle, m):
    """an all-zero structure PSSM: the structure score is exactly 0 and the sum IS the printed sequence score; T on the 0.001 grid"""
    rng = np.random.default_rng(77 + m)
    s = rand_stream(rng, 13, 200, 2500)
    T_tab, P = rand_table(rng, m), np.zeros((m, 7))
    motif = ctx.motif(T_tab, P)
    want_seq, want_st = oracle.stream_seq(s.codes, T_tab), oracle.stream_struct(s.profile, P)
    assert (want_st[np.isfinite(want_st)] == 0.0).all()
    printed = np.round(want_seq[np.isfinite(want_seq)], 3)
    grid = np.unique(printed[(printed > np.quantile(printed, 0.3)) & (printed < np.quantile(printed, 0.7))])
    ctx.stage(s.codes, s.profile)
    sizes = set()
    for v in rng.choice(grid, size=8, replace=False):
        T = round(float(v), 3)                             # the decimal on the grid, as a double: NOT the float32's value
        want_pos = want_hits(oracle, want_seq, want_st, -np.inf, -np.inf, T)
        pos, sq, st = ctx.hits_sum_staged(motif, -np.inf, -np.inf, T)
        assert np.array_equal(pos, want_pos), (T, pos.size, want_pos.size)
        assert_f32_bits_equal(sq, want_seq[want_pos])
        assert (st == 0.0).all()
        sizes.add(pos.size)
    assert len(sizes) > 1 and min(sizes) > 100
    motif.close()


# ---- the entry-point forms --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forms(oracle):
    rng = np.random.default_rng(808)
    s = rand_stream(rng, 14, 200, 2500)
    T_tab, P = rand_table(rng, 12), rand_struct_pssm(rng, 12)
    want_seq, want_st = oracle.stream_seq(s.codes, T_tab), oracle.stream_struct(s.profile, P)
    thr_seq, thr_st = quantiles(want_seq.astype(np.float64), [0.6])[0], quantiles(want_st, [0.2])[0]
    plain = oracle.stream_hits(want_seq, want_st, thr_seq, thr_st)
    T = quantiles(want_sum_of(want_seq, want_st)[plain], [0.5])[0]
    return dict(s=s, T_tab=T_tab, P=P, want_seq=want_seq, want_st=want_st, thr_seq=thr_seq, thr_st=thr_st, T=T, plain=plain,
                want_pos=want_hits(oracle, want_seq, want_st, thr_seq, thr_st, T))


def _dev_call(ctx, motif, f, thr_sum):
    import torch
    from rnascan_amd import _lib
    s = f["s"]
    codes, prof = torch.from_numpy(s.codes).to(DEV), torch.from_numpy(s.profile).to(DEV)
    cap = s.n_pos
    pos = torch.full((cap,), -1, dtype=torch.int64, device=DEV)
    sq = torch.zeros(cap, dtype=torch.float32, device=DEV)
    st = torch.zeros(cap, dtype=torch.float64, device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    if thr_sum is None:
        ctx.hits_dev(motif, codes.data_ptr(), prof.data_ptr(), _lib.PROFILE_F32, s.n_pos, f["thr_seq"], f["thr_st"], cap,
                     pos.data_ptr(), sq.data_ptr(), st.data_ptr(), count.data_ptr())
    else:
        ctx.hits_sum_dev(motif, codes.data_ptr(), prof.data_ptr(), _lib.PROFILE_F32, s.n_pos, f["thr_seq"], f["thr_st"], thr_sum, cap,
                         pos.data_ptr(), sq.data_ptr(), st.data_ptr(), count.data_ptr())
    ctx.synchronize()
    k = int(count.item())
    order = np.argsort(pos[:k].cpu().numpy(), kind="stable")
    return pos[:k].cpu().numpy()[order], sq[:k].cpu().numpy()[order], st[:k].cpu().numpy()[order]


@pytest.mark.parametrize("form", ["host", "staged", "pipeline", "dev"])
def test_form_gives_the_oracle_set_and_minus_inf_is_the_plain_call(ctx, forms, form):
    f = forms
    s = f["s"]
    motif = ctx.motif(f["T_tab"], f["P"])
    if form == "staged":
        ctx.stage(s.codes, s.profile)

    def plain_call():
        if form == "host":
            return ctx.hits_host(motif, s.codes, s.profile, f["thr_seq"], f["thr_st"])
        if form == "staged":
            return ctx.hits_staged(motif, f["thr_seq"], f["thr_st"])
        if form == "pipeline":                             # windows straddle the 4096-position chunk borders
            return ctx.hits_pipeline_host(motif, s.codes, s.profile, f["thr_seq"], f["thr_st"], chunk_positions=4096)
        return _dev_call(ctx, motif, f, None)

    def sum_call(T):
        if form == "host":
            return ctx.hits_sum_host(motif, s.codes, s.profile, f["thr_seq"], f["thr_st"], T)
        if form == "staged":
            return ctx.hits_sum_staged(motif, f["thr_seq"], f["thr_st"], T)
        if form == "pipeline":
            return ctx.hits_sum_pipeline_host(motif, s.codes, s.profile, f["thr_seq"], f["thr_st"], T, chunk_positions=4096)
        return _dev_call(ctx, motif, f, T)

    # thr_sum = -inf: exactly the hits of pfmscan_hits_*
    a, b = sum_call(-np.inf), plain_call()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])
    assert np.array_equal(b[0], f["plain"])
    # a finite thr_sum: the oracle's set
    assert s.n_pos > 3 * 4096 and 0 < f["want_pos"].size < f["plain"].size
    check(sum_call(f["T"]), f["want_pos"], f["want_seq"], s.profile, f["P"], form)
    borders = np.arange(4096, s.n_pos, 4096)
    assert any(((f["want_pos"] < b) & (f["want_pos"] + 12 > b)).any() for b in borders), "no hit window straddles a chunk border"
    motif.close()


class HitsSumDev(HitsDev):
    """pfmscan_hits_sum_dev in the pattern of test_gpu_dev_streams: behind a delay on the caller's side stream"""

    def __init__(self, ctx, oracle):
        HitsDev.__init__(self, ctx, oracle)
        plain = self.want_pos
        self.T = quantiles(want_sum_of(self.want_seq, self.want_st)[plain], [0.4])[0]
        self.want_pos = want_hits(oracle, self.want_seq, self.want_st, self.thr_seq, self.thr_st, self.T)
        assert 20 < self.want_pos.size < plain.size

    def call(self, buf, outs, stream, alt):
        self.ctx.hits_sum_dev(self.motif, buf["codes"].data_ptr(), buf["profile"].data_ptr(), self.dt, self.s.n_pos, self.thr_seq,
                              self.thr_st, self.T, self.s.n_pos, _ptr(outs, "pos"), _ptr(outs, "seq"), _ptr(outs, "st"),
                              _ptr(outs, "count"), stream)


def test_dev_form_runs_in_the_order_of_the_callers_stream(ctx, oracle, delay):    # noqa: F811
    import torch
    case = HitsSumDev(ctx, oracle)
    S = torch.cuda.Stream()
    try:
        own_ms, warm_outs = _timed_plain_run(case, S)
        with pytest.raises(AssertionError):              # what that run left behind is ANOTHER answer
            case.check(warm_outs, "the warm run", False)
        need_ms = max(20.0, 20.0 * own_ms)
        outs, pending, delay_ms = _behind_delay(case, delay, S, need_ms)
        msg = "delay %.1f ms (%.1f ms asked for; the call's own %.3f ms)" % (delay_ms, need_ms, own_ms)
        assert delay_ms >= need_ms, "the delay was too short for the test to mean anything: " + msg
        assert pending[0], "the call returned only after the work queued in front of it had run: not asynchronous; " + msg
        case.check(outs[0], msg, False)
    finally:
        torch.cuda.synchronize()
        case.close()


def test_capacity_protocol_and_rejections(ctx, forms):
    from rnascan_amd import _lib
    f = forms
    s = f["s"]
    motif = ctx.motif(f["T_tab"], f["P"])
    k = f["want_pos"].size
    assert k > 40
    # too small: PFMSCAN_E_CAPACITY, *n_hits a capacity that suffices, nothing written to the hit arrays
    cap = k // 3
    pos = np.full(cap, -7, dtype=np.int64)
    sq = np.full(cap, -7.0, dtype=np.float32)
    st = np.full(cap, -7.0, dtype=np.float64)
    n = ctypes.c_int64(0)
    prof = np.ascontiguousarray(s.profile)
    rc = ctx._L.pfmscan_hits_sum_host(ctx._h, motif._h, s.codes.ctypes.data, prof.ctypes.data, _lib.PROFILE_F32, s.n_pos,
                                      f["thr_seq"], f["thr_st"], f["T"], cap, pos.ctypes.data, sq.ctypes.data, st.ctypes.data,
                                      ctypes.byref(n))
    assert rc == _lib.E_CAPACITY and n.value >= k
    assert (pos == -7).all() and (sq == -7.0).all() and (st == -7.0).all()
    with pytest.raises(_lib.CapacityError):
        ctx.hits_sum_host(motif, s.codes, s.profile, f["thr_seq"], f["thr_st"], f["T"], capacity=cap)
    got = ctx.hits_sum_host(motif, s.codes, s.profile, f["thr_seq"], f["thr_st"], f["T"], capacity=int(n.value))
    assert np.array_equal(got[0], f["want_pos"])
    # NaN thr_sum; a motif with one part
    with pytest.raises(ValueError):
        ctx.hits_sum_host(motif, s.codes, s.profile, f["thr_seq"], f["thr_st"], float("nan"))
    with pytest.raises(ValueError):
        ctx.hits_sum_staged(motif, f["thr_seq"], f["thr_st"], float("nan"))
    for lt, pp in ((f["T_tab"], None), (None, f["P"])):
        one = ctx.motif(lt, pp)
        with pytest.raises(ValueError):
            ctx.hits_sum_host(one, s.codes if lt is not None else None, s.profile if pp is not None else None, -np.inf, -np.inf, 0.0)
        with pytest.raises(ValueError):
            ctx.hits_sum_pipeline_host(one, s.codes if lt is not None else None, s.profile if pp is not None else None, -np.inf, -np.inf, 0.0)
        one.close()
    motif.close()


# ---- the command line --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minscore", ["-6", " -inf"])        # -6: 450 rows of the three pairs; -inf: every window
def test_cli_on_the_gpu_equals_the_cli_on_the_oracle_engine(tmp_path, minscore):
    """a small store with 3 motif pairs of two widths: one hits_sum call per pair on the staged stream"""
    from engines import OracleEngine
    from rnascan_amd import cli, fasta, pssm, scanner, store
    from test_scanner_cpu import _library_inputs, assert_tsv_equal
    for seed in range(5, 40):                              # the first seed whose three pairs have two widths
        sub = tmp_path / ("in%d" % seed)
        sub.mkdir()
        lib_s, lib_t, fa, d = _library_inputs(sub, 3, seed)
        if len({p.length for p in pssm.load_pssms(lib_s, 0.01, fasta.RNA, None).values()}) == 2:
            break
    else:
        raise AssertionError("no seed gives two widths")
    sdir = str(tmp_path / "store")
    assert store.main([d, sdir]) == 0

    def run(argv, engine):
        out = io.StringIO()
        cli.main(argv, engine=engine, out=out)
        return out.getvalue()

    base = ["-p", lib_s, "-q", lib_t, "-u", "-C", "0.01", "-m", minscore]
    plain = run(base + [fa, sdir], OracleEngine())
    at = plain.splitlines()[0].split("\t").index("LogOdds.SeqStruct")
    sums = np.array([float(l.split("\t")[at]) for l in plain.splitlines()[1:]])
    assert sums.size > 50
    T = repr(float(np.sort(sums)[sums.size // 2]))
    want = run(base + ["--min-seqstruct", T, fa, sdir], OracleEngine())
    engine = scanner.HipEngine(0)
    try:
        got = run(base + ["--min-seqstruct", T, fa, sdir], engine)
    finally:
        engine.close()
    assert 10 < want.count("\n") < plain.count("\n")
    assert_tsv_equal(got, want, tol=1e-6)
