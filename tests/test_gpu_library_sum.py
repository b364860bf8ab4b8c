"""PFM libraries with the joint threshold on LogOdds.SeqStruct decided in the library kernel (pfmscan_library_hits_sum_*,
k_library<.., SUM>) and the row bound it rests on (pfmscan_profile_row_bound_*).

The oracle for every hit set: pair k keeps window p iff seq_k(p) > thr_seq[k] and struct_k(p) > thr_struct[k] and the printed
sum float64(np.round(float32 seq, 3)) + struct exceeds T[k] (strict; NaN never passes), scores from the CPU oracle one motif
at a time.  Phase A's credits are built for thr_eff = max(thr_seq, T - the bound on a structure score), so thr_seq may be
-inf; phase B decides with the caller's thresholds.  Sets are exact, reported seq is bit-equal, reported struct lies within
its rounding-error bound."""
import ctypes
import io

import numpy as np
import pytest

from conftest import assert_f32_bits_equal
from precision_rules import assert_struct_tight
from test_gpu_dev_streams import DEV, LibraryCombined, _behind_delay, _ptr, _timed_plain_run, delay    # noqa: F401 (delay: a fixture)
from test_gpu_library import _below_max, _clear_of, make_library, quantile_thresholds
from test_gpu_parity import rand_stream, rand_struct_pssm, rand_table
from test_gpu_sum_hits import _planted, want_sum_of
from test_library_sum_cpu import row_bound_np

pytestmark = pytest.mark.gpu


# ---- the oracle ------------------------------------------------------------------------------------------------------------
class Scores(object):
    """the oracle's scores of every motif of a library over a stream, computed once and shared"""

    def __init__(self, oracle, s, T, P):
        self.oracle, self.s, self.T, self.P = oracle, s, T, P
        self.sq = [oracle.stream_seq(s.codes, T[k]) for k in range(T.shape[0])]
        self.st = [oracle.stream_struct(s.profile, P[k]) for k in range(T.shape[0])]
        self.sums = [want_sum_of(a, b) for a, b in zip(self.sq, self.st)]

    def hits(self, ts, tt, tj=None):
        """(pos, motif, seq, struct) sorted by (pos, motif); tj None: without the joint threshold"""
        n = len(self.sq)
        ts, tt = np.broadcast_to(np.asarray(ts, dtype=np.float64), (n,)), np.broadcast_to(np.asarray(tt, dtype=np.float64), (n,))
        pos, mo, sq, st = [], [], [], []
        for k in range(n):
            p = self.oracle.stream_hits(self.sq[k], self.st[k], ts[k], tt[k])
            if tj is not None:
                with np.errstate(invalid="ignore"):
                    p = p[self.sums[k][p] > np.broadcast_to(np.asarray(tj, dtype=np.float64), (n,))[k]]
            pos.append(p)
            mo.append(np.full(p.size, k, dtype=np.int32))
            sq.append(self.sq[k][p])
            st.append(self.st[k][p])
        pos, mo, sq, st = np.concatenate(pos), np.concatenate(mo), np.concatenate(sq), np.concatenate(st)
        order = np.lexsort((mo, pos))
        return pos[order], mo[order], sq[order], st[order]

    def count(self, ts, tt):
        """the number of hits without the joint threshold"""
        n = len(self.sq)
        ts, tt = np.broadcast_to(np.asarray(ts, dtype=np.float64), (n,)), np.broadcast_to(np.asarray(tt, dtype=np.float64), (n,))
        return sum(self.oracle.stream_hits(self.sq[k], self.st[k], ts[k], tt[k]).size for k in range(n))

    def quantile_thresholds(self, q_seq, q_struct):
        """test_gpu_library.quantile_thresholds from the scores held here"""
        n = len(self.sq)
        ts, tt = np.empty(n), np.empty(n)
        for k in range(n):
            sq = self.sq[k].astype(np.float64)
            ts[k] = _below_max(sq[np.isfinite(sq)], q_seq)
            fin = self.st[k][np.isfinite(self.st[k]) & (np.abs(self.st[k]) < 1e9)]
            tt[k] = _clear_of(fin, _below_max(fin, q_struct))
        return ts, tt

    def sum_quantiles(self, ts, tt, rng, lo=0.2, hi=0.8, most=400):
        """a different T per motif: a quantile of the printed sums of ITS plain hits, between lo and hi -- higher where that
        would leave more than about `most` hits per motif (the checks below look at every hit)"""
        n = len(self.sq)
        ts, tt = np.broadcast_to(np.asarray(ts, dtype=np.float64), (n,)), np.broadcast_to(np.asarray(tt, dtype=np.float64), (n,))
        tj = np.zeros(n)
        for k in range(n):
            p = self.oracle.stream_hits(self.sq[k], self.st[k], ts[k], tt[k])
            v = self.sums[k][p]
            v = v[np.isfinite(v) & (np.abs(v) < 1e300)]
            if v.size:
                q = rng.uniform(lo, hi)
                tj[k] = float(np.quantile(v, max(q, 1.0 - most * (0.5 + 0.5 * q) / v.size)))
        return tj


def check(got, want, s, P, what=""):
    pos, mo, sq, st = got
    wp, wm, wsq, _ = want
    assert len(pos) == len(wp), "%d hits, the oracle has %d; %s" % (len(pos), len(wp), what)
    assert np.array_equal(pos, wp) and np.array_equal(mo, wm), what
    assert_f32_bits_equal(sq, wsq)
    for k in np.unique(wm):
        sel = wm == k
        assert_struct_tight(st[sel], s.profile, P[k], positions=wp[sel])


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)) and \
        np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64))


# ---- hit sets ---------------------------------------------------------------------------------------------------------------
# (n, m): one and two groups of 12 motifs (10-bit credits), 16-bit credits (m = 18), the wide buckets (33, 64), several
# passes (130 x 12; one after the other: teams need a long stream, test_gpu_library_teams.py)
SHAPES = [(2, 12), (13, 12), (25, 8), (9, 18), (10, 33), (10, 64), (130, 12)]


def _stream(rng, kind, dtype):
    if kind == "small":                                    # ~24 records <= 900 positions: under one 16 384-window segment
        return rand_stream(rng, 24, 0, 900, foreign=0.004, dtype=dtype)
    return rand_stream(rng, 60, 500, 3000, foreign=0.002, dtype=dtype)       # several segments and workgroups


def hit_set_case(oracle, n, m, kind, dtype):
    """-> (stream, T, P, Scores, [(thr_seq, thr_struct, T per motif, want with T, plain count)]) for the four threshold combinations"""
    rng = np.random.default_rng(7000 + 100 * n + m + (1 if kind == "long" else 0) + (2 if dtype == np.float64 else 0))
    s = _stream(rng, kind, dtype)
    T, P = make_library(rng, n, m)
    sc = Scores(oracle, s, T, P)
    qs, qt = sc.quantile_thresholds(0.9, 0.3)
    combos = []
    for ts in (qs, np.full(n, -np.inf)):
        for tt in (qt, np.full(n, -np.inf)):
            tj = sc.sum_quantiles(ts, tt, rng, most=min(400, 20000 // n))
            combos.append((ts, tt, tj, sc.hits(ts, tt, tj), sc.count(ts, tt)))
    return s, T, P, sc, combos


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["small", "long"])
@pytest.mark.parametrize("n,m", SHAPES)
def test_hit_sets_equal_the_oracle_and_the_per_pair_route(ctx, oracle, n, m, kind, dtype):
    s, T, P, sc, combos = hit_set_case(oracle, n, m, kind, dtype)
    lib = ctx.library(T, P)
    ctx.stage(s.codes, s.profile)
    assert np.isfinite(ctx.profile_row_bound_staged())
    for ts, tt, tj, want, n_plain in combos:
        assert 0 < len(want[0]) < n_plain, (len(want[0]), n_plain)
        got = ctx.library_hits_sum_staged(lib, ts, tt, tj)
        check(got, want, s, P, (n, m, kind, ts[0], tt[0]))
    # the parent's route, one hits_sum_staged per pair, in all four threshold combinations: the same sets (every pair of a
    # library of up to 13, else 13 spread over it, the first and the last among them)
    pairs = sorted(set(int(round(i * (n - 1) / 12.0)) for i in range(13))) if n > 13 else range(n)
    motifs = {k: ctx.motif(T[k], P[k]) for k in pairs}
    for ts, tt, tj, want, _ in combos:
        got = ctx.library_hits_sum_staged(lib, ts, tt, tj)
        for k in pairs:
            pos, sq, st = ctx.hits_sum_staged(motifs[k], ts[k], tt[k], tj[k])
            sel = got[1] == k
            assert np.array_equal(got[0][sel], pos)
            assert_f32_bits_equal(got[2][sel], sq)
            assert_struct_tight(got[3][sel], s.profile, P[k], positions=pos)
    for mo in motifs.values():
        mo.close()
    lib.close()


def test_tiny_and_empty_streams(ctx, oracle):
    """the streams of test_library_on_tiny_and_empty_streams: no window fits / nothing staged / one window"""
    from rnascan_amd import pack
    rng = np.random.default_rng(2)
    T, P = make_library(rng, 10, 12)
    lib = ctx.library(T, P)
    halved = 0
    for lengths in ([], [0], [3, 0, 11], [12], [5, 12, 13]):
        codes = [rng.integers(0, 4, size=L).astype(np.uint8) for L in lengths]
        profs = [rng.dirichlet(np.full(7, 0.3), size=L).astype(np.float32) if L else np.zeros((0, 7), np.float32) for L in lengths]
        if not lengths:                                    # an empty stream has no hits (and is no error)
            got = ctx.library_hits_sum_host(lib, np.zeros(0, np.uint8), np.zeros((0, 7), np.float32), -np.inf, -np.inf, 0.0)
            assert len(got[0]) == 0
            continue
        s = pack.pack(codes, profs)
        sc = Scores(oracle, s, T, P)
        allsums = np.concatenate(sc.sums)
        allsums = allsums[np.isfinite(allsums)]
        tj = float(np.median(allsums)) if allsums.size else 0.0          # one T for all ten motifs: about half of the windows
        want, plain = sc.hits(-np.inf, -np.inf, tj), sc.hits(-np.inf, -np.inf)
        assert len(plain[0]) == 10 * sum(max(L - 11, 0) for L in lengths)
        got = ctx.library_hits_sum_host(lib, s.codes, s.profile, -np.inf, -np.inf, tj)
        check(got, want, s, P, lengths)
        if len(plain[0]):
            assert 0 < len(want[0]) < len(plain[0])
            halved += 1
    assert halved == 2
    lib.close()


# ---- thresholds planted ON a window's printed sum and one ulp beside it ------------------------------------------------------
class LibraryAsMotif(object):
    """what test_gpu_sum_hits._planted needs of a context, answered by the LIBRARY route: the planted motif is pair `slot` of a
    library whose other pairs carry thresholds of their own"""

    class Handle(object):
        def __init__(self, real, lib):
            self.real, self.lib = real, lib

        def close(self):
            self.real.close()
            self.lib.close()

    def __init__(self, ctx, rng, n, slot):
        self.ctx, self.rng, self.n, self.slot = ctx, rng, n, slot

    def motif(self, T_tab, P):
        m = T_tab.shape[0]
        LT, LP = make_library(self.rng, self.n, m)
        LT[self.slot], LP[self.slot] = T_tab, P
        self.others = self.rng.normal(4.0, 2.0, size=self.n)        # high: the other pairs keep a few per cent of their windows
        return LibraryAsMotif.Handle(self.ctx.motif(T_tab, P), self.ctx.library(LT, LP))

    def scan_host(self, motif, codes, profile):
        return self.ctx.scan_host(motif.real, codes, profile)

    def hits_sum_host(self, motif, codes, profile, thr_seq, thr_st, T):
        tj = self.others.copy()
        tj[self.slot] = T
        # room for every window of the planted pair and the few of the others: the stream is one or two work segments, and a
        # capacity found by the retry protocol is sized for the fullest shard times all 256
        pos, mo, sq, st = self.ctx.library_hits_sum_host(motif.lib, codes, profile, thr_seq, thr_st, tj, capacity=3 * codes.size)
        sel = mo == self.slot
        return pos[sel], sq[sel], st[sel]


@pytest.mark.parametrize("cells", ["finite", "inf"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m", [12, 18])
def test_thresholds_on_and_beside_the_sum(ctx, oracle, m, dtype, cells):
    from test_gpu_sum_hits import struct_pssm
    rng = np.random.default_rng(5100 + m + (1 if dtype == np.float64 else 0) + (2 if cells == "inf" else 0))
    s = rand_stream(rng, 12, 200, 2500, dtype=dtype)
    T_tab, P = rand_table(rng, m), struct_pssm(rng, m, cells)
    # (with float32 rows or -inf cells the two orders agree almost everywhere, as for the structure threshold)
    need = 4 if (cells == "finite" and dtype == np.float64) else 0
    _planted(oracle, LibraryAsMotif(ctx, rng, 13, 5), s, T_tab, P, -np.inf, -np.inf, rng, need)


@pytest.mark.parametrize("m", [12, 18])
def test_rounding_grid_through_phase_b(ctx, oracle, m):
    """all-zero structure PSSMs: the structure score is exactly 0, its bound is 0 and the sum IS the printed sequence score --
    thr_eff sits 0.0005 (and the rounding terms) under T, so the windows that decide are phase A's survivors; T on the
    0.001 grid, where round3 ties are"""
    rng = np.random.default_rng(177 + m)
    s = rand_stream(rng, 13, 200, 2500)
    n = 5
    T, _ = make_library(rng, n, m)
    P = np.zeros((n, m, 7))
    sc = Scores(oracle, s, T, P)
    lib = ctx.library(T, P)
    ctx.stage(s.codes, s.profile)
    sizes = set()
    for _ in range(6):
        tj = np.empty(n)
        for k in range(n):
            printed = np.round(sc.sq[k][np.isfinite(sc.sq[k])], 3)
            grid = np.unique(printed[(printed > np.quantile(printed, 0.9)) & (printed < np.quantile(printed, 0.99))])
            tj[k] = round(float(rng.choice(grid)), 3)      # the decimal on the grid, as a double: NOT the float32's value
        eff = ctx_eff(ctx, T, P, -np.inf, tj)
        assert ((tj - eff > 0.0005) & (tj - eff < 0.0006)).all()
        want = sc.hits(-np.inf, -np.inf, tj)
        got = ctx.library_hits_sum_staged(lib, -np.inf, -np.inf, tj)
        check(got, want, s, P, tj)
        assert (got[3] == 0.0).all()
        sizes.add(len(got[0]))
    assert len(sizes) > 1 and min(sizes) > 100
    assert lib.info()["max_prefilter_eps"] < np.inf
    lib.close()


def ctx_eff(ctx, T, P, thr_seq, tj):
    from rnascan_amd import _lib
    return _lib.library_sum_thresholds(T, P, thr_seq, tj, ctx.profile_row_bound_staged())


# ---- the entry-point forms ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forms(oracle):
    rng = np.random.default_rng(909)
    s = rand_stream(rng, 14, 200, 2500)
    T, P = make_library(rng, 13, 12)
    sc = Scores(oracle, s, T, P)
    ts, tt = quantile_thresholds(oracle, s, T, P, 0.9, 0.3)
    tj = sc.sum_quantiles(ts, tt, rng, 0.3, 0.5, most=10 ** 9)
    tj2 = sc.sum_quantiles(ts, tt, rng, 0.6, 0.8, most=10 ** 9)
    f = dict(s=s, T=T, P=P, sc=sc, ts=ts, tt=tt, tj=tj, tj2=tj2, plain=sc.hits(ts, tt), want=sc.hits(ts, tt, tj), want2=sc.hits(ts, tt, tj2),
             S=row_bound_np(s.codes, s.profile))
    assert 0 < len(f["want2"][0]) < len(f["want"][0]) < len(f["plain"][0])
    return f


def _dev_call(ctx, lib, f, tj, S=None):
    """pfmscan_library_hits_dev (tj None) or pfmscan_library_hits_sum_dev on torch tensors -> sorted numpy arrays"""
    import torch
    from rnascan_amd import _lib
    s = f["s"]
    codes, prof = torch.from_numpy(s.codes).to(DEV), torch.from_numpy(s.profile).to(DEV)
    cap = len(f["plain"][0]) + 64
    pos = torch.full((cap,), -1, dtype=torch.int64, device=DEV)
    mo = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
    sq = torch.zeros(cap, dtype=torch.float32, device=DEV)
    st = torch.zeros(cap, dtype=torch.float64, device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    if tj is None:
        ctx.library_hits_dev(lib, codes.data_ptr(), prof.data_ptr(), _lib.PROFILE_F32, s.n_pos, f["ts"], f["tt"], cap,
                             pos.data_ptr(), mo.data_ptr(), sq.data_ptr(), st.data_ptr(), count.data_ptr())
    else:
        ctx.library_hits_sum_dev(lib, codes.data_ptr(), prof.data_ptr(), _lib.PROFILE_F32, s.n_pos, f["ts"], f["tt"], tj, S, cap,
                                 pos.data_ptr(), mo.data_ptr(), sq.data_ptr(), st.data_ptr(), count.data_ptr())
    ctx.synchronize()
    k = int(count.item())
    assert k <= cap
    pos, mo, sq, st = pos[:k].cpu().numpy(), mo[:k].cpu().numpy(), sq[:k].cpu().numpy(), st[:k].cpu().numpy()
    order = np.lexsort((mo, pos))
    return pos[order], mo[order], sq[order], st[order]


@pytest.mark.parametrize("form", ["host", "staged", "dev"])
def test_form_gives_the_oracle_set_and_minus_inf_is_the_plain_call(ctx, forms, form):
    f = forms
    s = f["s"]
    lib = ctx.library(f["T"], f["P"])
    if form == "staged":
        ctx.stage(s.codes, s.profile)

    def plain_call():
        if form == "host":
            return ctx.library_hits_host(lib, s.codes, s.profile, f["ts"], f["tt"])
        if form == "staged":
            return ctx.library_hits_staged(lib, f["ts"], f["tt"])
        return _dev_call(ctx, lib, f, None)

    def sum_call(tj):
        if form == "host":
            return ctx.library_hits_sum_host(lib, s.codes, s.profile, f["ts"], f["tt"], tj)
        if form == "staged":
            return ctx.library_hits_sum_staged(lib, f["ts"], f["tt"], tj)
        return _dev_call(ctx, lib, f, tj, f["S"])

    # thr_sum = -inf for every pair: the plain kernels, the plain call's hits bit for bit
    a, b = sum_call(np.full(13, -np.inf)), plain_call()
    assert same_bits(a, b)
    assert np.array_equal(b[0], f["plain"][0]) and np.array_equal(b[1], f["plain"][1])
    check(sum_call(f["tj"]), f["want"], s, f["P"], form)
    # some pairs without a joint threshold beside pairs with one
    mixed = f["tj"].copy()
    mixed[::3] = -np.inf
    check(sum_call(mixed), f["sc"].hits(f["ts"], f["tt"], mixed), s, f["P"], form + " mixed")
    lib.close()


def test_credit_tables_are_never_shared_between_different_effective_thresholds(ctx, oracle):
    """Structure PSSMs with small cells: the bound on a structure score is ~1.5, so thr_eff sits just under T and phase A's
    credits drop most windows -- windows that ARE hits of a plain call with the same thr_seq / thr_struct, or of a sum call with
    a lower T.  Each call must get tables built for ITS effective thresholds."""
    rng = np.random.default_rng(911)
    s = rand_stream(rng, 8, 200, 1500)
    T, P = make_library(rng, 13, 12)
    P *= 0.05
    sc = Scores(oracle, s, T, P)
    lib = ctx.library(T, P)
    ctx.stage(s.codes, s.profile)
    low = np.full(13, -3.0)                                # finite, under every thr_eff: the sum calls tighten it
    tt = np.full(13, -np.inf)
    tj = np.array([np.quantile(v[np.isfinite(v)], 0.9) for v in sc.sums])
    tj2 = np.array([np.quantile(v[np.isfinite(v)], 0.97) for v in sc.sums])
    eff, eff2 = ctx_eff(ctx, T, P, low, tj), ctx_eff(ctx, T, P, low, tj2)
    assert (eff > low + 1.0).all() and (eff2 > eff + 1.0).all() and (tj - eff < 2.5).all()
    plain, want, want2 = sc.hits(low, tt), sc.hits(low, tt, tj), sc.hits(low, tt, tj2)
    assert 0 < len(want2[0]) < len(want[0]) < len(plain[0])
    # hits of the plain call, and of the first sum call, that credits built for the second sum call would drop
    for w, e in ((plain, eff2), (plain, eff), (want, eff2)):
        assert all((sc.sq[k][w[0][w[1] == k]].astype(np.float64) <= e[k]).sum() > 10 for k in range(13))
    # sum then plain
    check(ctx.library_hits_sum_staged(lib, low, tt, tj2), want2, s, P, "sum")
    check(ctx.library_hits_staged(lib, low, tt), plain, s, P, "plain after sum")
    # plain then sum
    check(ctx.library_hits_sum_staged(lib, low, tt, tj), want, s, P, "sum after plain")
    # two sum calls with different T: the tighter one, then the other again
    check(ctx.library_hits_sum_staged(lib, low, tt, tj2), want2, s, P, "sum 2")
    check(ctx.library_hits_sum_staged(lib, low, tt, tj), want, s, P, "sum 1 after sum 2")
    # thr_seq = -inf reaches the kernel through thr_eff alone
    check(ctx.library_hits_sum_staged(lib, -np.inf, tt, tj2), sc.hits(-np.inf, tt, tj2), s, P, "thr_seq = -inf")
    lib.close()


class LibrarySumDev(LibraryCombined):
    """pfmscan_library_hits_sum_dev in the pattern of test_gpu_dev_streams: behind a delay on the caller's side stream; the
    repeated call stays asynchronous, the call with other thresholds gets its own tables"""

    def __init__(self, ctx, oracle):
        LibraryCombined.__init__(self, ctx, oracle)
        sc = Scores(oracle, self.s, self.LT, self.LP)
        rng = np.random.default_rng(3)
        self.S = row_bound_np(self.s.codes, self.s.profile)
        self.tj = [sc.sum_quantiles(ts, tt, rng, 0.3, 0.6) for ts, tt in self.thr]
        plain = self.want
        self.want = [sc.hits(ts, tt, tj) for (ts, tt), tj in zip(self.thr, self.tj)]
        assert all(20 < len(w[0]) < len(p[0]) for w, p in zip(self.want, plain))

    def call(self, buf, outs, stream, alt):
        ts, tt = self.thr[int(alt)]
        self.ctx.library_hits_sum_dev(self.lib, buf["codes"].data_ptr(), buf["profile"].data_ptr(), self.dt, self.s.n_pos, ts, tt,
                                      self.tj[int(alt)], self.S, self.cap, _ptr(outs, "pos"), _ptr(outs, "motif"), _ptr(outs, "seq"),
                                      _ptr(outs, "st"), _ptr(outs, "count"), stream)

    def check(self, out, msg, alt):
        want = self.want[int(alt)]
        got = self._sorted(out, len(want[0]), msg)
        check(got, want, self.s, self.LP, msg)


def test_dev_form_runs_in_the_order_of_the_callers_stream(ctx, oracle, delay):    # noqa: F811
    import torch
    case = LibrarySumDev(ctx, oracle)
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
        assert pending[1], "the repeated call with the same thresholds was not asynchronous; " + msg
        case.check(outs[1], "repeated call; " + msg, False)
        case.check(outs[2], "call with other thresholds; " + msg, True)
    finally:
        torch.cuda.synchronize()
        case.close()


# ---- the promise about the rows ----------------------------------------------------------------------------------------------
def _broken_stream(rng, under_separators):
    """a negative cell, a NaN cell and a row of sum 3, each inside a record -- or each under a code-7 position"""
    s = rand_stream(rng, 14, 300, 2000, foreign=0.003)
    inside = np.flatnonzero((s.codes & 7) != 7)
    inside = inside[(inside > 50) & (inside < s.n_pos - 50)]
    sep = np.flatnonzero((s.codes & 7) == 7)
    rows = (rng.choice(sep, size=3, replace=False) if under_separators else rng.choice(inside, size=3, replace=False))
    s.profile[rows[0], 2] = -0.25
    s.profile[rows[1], 5] = np.nan
    s.profile[rows[2]] = 0.0
    s.profile[rows[2], :3] = 1.0
    return s, rows


def test_rows_that_break_the_promise(ctx, oracle):
    from rnascan_amd import _lib
    rng = np.random.default_rng(31)
    T, P = make_library(rng, 13, 12)
    lib = ctx.library(T, P)
    for rows_kept in ([2], [0, 1, 2]):                      # only the row of sum 3 (S = 3); all three (S = inf)
        s, rows = _broken_stream(rng, False)
        for r in set([0, 1, 2]) - set(rows_kept):
            s.profile[rows[r]] = 1.0 / 7
        sc = Scores(oracle, s, T, P)
        ctx.stage(s.codes, s.profile)
        S = ctx.profile_row_bound_staged()
        assert S == (3.0 if rows_kept == [2] else np.inf) and S == row_bound_np(s.codes, s.profile)
        ts, tt = quantile_thresholds(oracle, s, T, P, 0.9, 0.3)
        tj = sc.sum_quantiles(ts, tt, rng)
        want, plain = sc.hits(ts, tt, tj), sc.hits(ts, tt)
        assert 0 < len(want[0]) < len(plain[0])
        # a finite thr_seq: no hit is dropped, whatever the rows hold (S = inf: no tightening at all)
        check(ctx.library_hits_sum_staged(lib, ts, tt, tj), want, s, P, rows_kept)
        if np.isfinite(S):
            tj_inf = sc.sum_quantiles(np.full(13, -np.inf), tt, rng)
            check(ctx.library_hits_sum_staged(lib, -np.inf, tt, tj_inf), sc.hits(-np.inf, tt, tj_inf), s, P, "S = 3, thr_seq = -inf")
            continue
        # thr_seq = -inf and S = inf: no finite letters threshold -> PFMSCAN_E_BADARG, nothing written
        with pytest.raises(ValueError, match="finite sequence threshold"):
            ctx.library_hits_sum_staged(lib, -np.inf, tt, tj)
        cap = 64
        pos, mo = np.full(cap, -7, dtype=np.int64), np.full(cap, -7, dtype=np.int32)
        sq, st = np.full(cap, -7.0, dtype=np.float32), np.full(cap, -7.0, dtype=np.float64)
        k = ctypes.c_int64(-5)
        neg = np.full(13, -np.inf)
        rc = ctx._L.pfmscan_library_hits_sum_staged(ctx._h, lib._h, neg.ctypes.data, tt.ctypes.data, tj.ctypes.data, cap, pos.ctypes.data,
                                                    mo.ctypes.data, sq.ctypes.data, st.ctypes.data, ctypes.byref(k))
        assert rc == _lib.E_BADARG and k.value <= 0
        assert (pos == -7).all() and (mo == -7).all() and (sq == -7.0).all() and (st == -7.0).all()
    # the same bad rows under code 7: ignored
    s, rows = _broken_stream(rng, True)
    sc = Scores(oracle, s, T, P)
    ctx.stage(s.codes, s.profile)
    S = ctx.profile_row_bound_staged()
    assert np.isfinite(S) and S < 1.001 and S == row_bound_np(s.codes, s.profile)
    tj = sc.sum_quantiles(-np.inf, -np.inf, rng)
    want = sc.hits(-np.inf, -np.inf, tj)
    assert 0 < len(want[0]) < len(sc.hits(-np.inf, -np.inf)[0])
    check(ctx.library_hits_sum_staged(lib, -np.inf, -np.inf, tj), want, s, P, "under separators")
    # NaN thresholds, a NaN promise, libraries of another kind
    with pytest.raises(ValueError):
        ctx.library_hits_sum_staged(lib, 0.0, 0.0, np.nan)
    lib.close()
    for kind in ("seq", "struct"):
        other = ctx.library(T if kind == "seq" else None, P if kind == "struct" else None)
        with pytest.raises(ValueError):
            ctx.library_hits_sum_staged(other, 0.0, 0.0, 0.0)
        other.close()


# ---- the row bound ---------------------------------------------------------------------------------------------------------
TILE = 256


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_row_bound_equals_its_numpy_restatement(ctx, dtype):
    import torch
    from rnascan_amd import _lib
    rng = np.random.default_rng(12 + (1 if dtype == np.float64 else 0))
    dt = _lib.PROFILE_F32 if dtype == np.float32 else _lib.PROFILE_F64
    sizes = [1, TILE - 1, TILE, TILE + 1, 5 * TILE + 3] + ([2 * 8 * 256 * TILE + 3] if dtype == np.float32 else [])     # the last: more tiles than workgroups
    seen = set()
    for n_pos in sizes:
        for variant in ("clean", "garbage under 7", "bad row"):
            prof = rng.dirichlet(np.full(7, 0.3), size=n_pos).astype(dtype)
            prof[rng.integers(0, n_pos)] *= 1.0 + rng.random()                       # one row above the others
            codes = rng.integers(0, 4, size=n_pos).astype(np.uint8)
            codes[rng.random(n_pos) < 0.3] |= 8                                      # bit 3 (lower case) does not count
            if variant != "clean":
                sep = np.flatnonzero(rng.random(n_pos) < 0.2)
                codes[sep] = 7 | (rng.integers(0, 2, size=sep.size).astype(np.uint8) << 3)
                if sep.size:
                    prof[sep] = rng.choice(np.array([np.nan, -1.0, 1e30, np.inf, 7.5], dtype=dtype), size=(sep.size, 7))
            if variant == "bad row":
                ok = np.flatnonzero((codes & 7) != 7)
                if ok.size:
                    prof[rng.choice(ok), rng.integers(0, 7)] = rng.choice(np.array([np.nan, -1e-30, np.inf], dtype=dtype))
            want = row_bound_np(codes, prof)
            ctx.stage(codes, prof)
            got = ctx.profile_row_bound_staged()
            assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (n_pos, variant, got, want)
            assert ctx.profile_row_bound_staged() == got                              # the cached value
            d_codes, d_prof = torch.from_numpy(codes).to(DEV), torch.from_numpy(prof).to(DEV)
            out = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
            ctx.profile_row_bound_dev(d_codes.data_ptr(), d_prof.data_ptr(), dt, n_pos, out.data_ptr())
            ctx.synchronize()
            assert np.float64(out.item()).view(np.uint64) == np.float64(want).view(np.uint64), (n_pos, variant, "dev")
            # without codes every row counts
            ctx.profile_row_bound_dev(None, d_prof.data_ptr(), dt, n_pos, out.data_ptr())
            ctx.synchronize()
            assert np.float64(out.item()).view(np.uint64) == np.float64(row_bound_np(None, prof)).view(np.uint64)
            seen.add(want)
    assert np.inf in seen and len(seen) > len(sizes)
    # all rows under code 7; an empty stream
    prof = np.full((9, 7), np.nan, dtype=dtype)
    ctx.stage(np.full(9, 7, dtype=np.uint8), prof)
    assert ctx.profile_row_bound_staged() == 0.0
    ctx.stage(np.zeros(0, np.uint8), np.zeros((0, 7), dtype))
    assert ctx.profile_row_bound_staged() == 0.0


# ---- capacity ----------------------------------------------------------------------------------------------------------------
def test_capacity_protocol(ctx, forms):
    from rnascan_amd import _lib
    f = forms
    s = f["s"]
    lib = ctx.library(f["T"], f["P"])
    k = len(f["want"][0])
    assert k > 40
    cap = k // 3
    pos, mo = np.full(cap, -7, dtype=np.int64), np.full(cap, -7, dtype=np.int32)
    sq, st = np.full(cap, -7.0, dtype=np.float32), np.full(cap, -7.0, dtype=np.float64)
    n = ctypes.c_int64(0)
    prof = np.ascontiguousarray(s.profile)
    rc = ctx._L.pfmscan_library_hits_sum_host(ctx._h, lib._h, s.codes.ctypes.data, prof.ctypes.data, _lib.PROFILE_F32, s.n_pos,
                                              f["ts"].ctypes.data, f["tt"].ctypes.data, f["tj"].ctypes.data, cap, pos.ctypes.data,
                                              mo.ctypes.data, sq.ctypes.data, st.ctypes.data, ctypes.byref(n))
    assert rc == _lib.E_CAPACITY and n.value >= k
    assert (pos == -7).all() and (mo == -7).all() and (sq == -7.0).all() and (st == -7.0).all()
    with pytest.raises(_lib.CapacityError):
        ctx.library_hits_sum_host(lib, s.codes, s.profile, f["ts"], f["tt"], f["tj"], capacity=cap)
    got = ctx.library_hits_sum_host(lib, s.codes, s.profile, f["ts"], f["tt"], f["tj"], capacity=int(n.value))
    check(got, f["want"], s, f["P"], "retry")
    lib.close()


# ---- the command line --------------------------------------------------------------------------------------------------------
def test_cli_takes_the_library_route(tmp_path, monkeypatch):
    """`-p lib13 -q lib13 seqs.fa store/ -m ' -inf' --min-seqstruct T`: every width group of the 13 pairs is ONE library_hits_sum
    call and hits_sum is never called.  Against the oracle-backed engine every field is the same text except the two unrounded
    fp64 structure columns, which the device computes with fused multiply-adds (within 1e-9, test_scanner_cpu.assert_tsv_equal);
    against the per-pair route of the same device the bytes are equal."""
    from engines import OracleEngine
    from rnascan_amd import cli, fasta, pssm, scanner, store
    from test_scanner_cpu import _library_inputs, assert_tsv_equal
    for seed in range(5, 60):                              # the first seed whose 13 pairs leave no width alone
        sub = tmp_path / ("in%d" % seed)
        sub.mkdir()
        lib_s, lib_t, fa, d = _library_inputs(sub, 13, seed)
        widths = [p.length for p in pssm.load_pssms(lib_s, 0.01, fasta.RNA, None).values()]
        if len(set(widths)) >= 2 and min(widths.count(w) for w in set(widths)) >= 2:
            break
    else:
        raise AssertionError("no seed gives width groups of two pairs or more")
    sdir = str(tmp_path / "store")
    assert store.main([d, sdir]) == 0

    def run(argv, engine):
        out = io.StringIO()
        cli.main(argv, engine=engine, out=out)
        return out.getvalue()

    base = ["-p", lib_s, "-q", lib_t, "-u", "-C", "0.01", "-m", " -inf"]
    plain = run(base + [fa, sdir], OracleEngine())
    at = plain.splitlines()[0].split("\t").index("LogOdds.SeqStruct")
    sums = np.array([float(l.split("\t")[at]) for l in plain.splitlines()[1:]])
    assert sums.size > 500
    T = repr(float(np.sort(sums)[int(sums.size * 0.9)]))
    want = run(base + ["--min-seqstruct", T, fa, sdir], OracleEngine())
    calls = {"library_hits_sum": 0, "hits_sum": 0}
    for name in calls:
        def counted(self, *a, _name=name, _real=getattr(scanner.HipEngine, name), **kw):
            calls[_name] += 1
            return _real(self, *a, **kw)
        monkeypatch.setattr(scanner.HipEngine, name, counted)
    engine = scanner.HipEngine(0)
    try:
        got = run(base + ["--min-seqstruct", T, fa, sdir], engine)
    finally:
        engine.close()
    assert 10 < want.count("\n") < plain.count("\n")
    assert calls == {"library_hits_sum": len(set(widths)), "hits_sum": 0}
    assert_tsv_equal(got, want)
    # the parent's route on the same device: one hits_sum per pair -- the same bytes
    monkeypatch.delattr(scanner.HipEngine, "library_hits_sum")
    engine = scanner.HipEngine(0)
    try:
        per_pair = run(base + ["--min-seqstruct", T, fa, sdir], engine)
    finally:
        engine.close()
    assert calls["hits_sum"] == 13
    assert per_pair == got
