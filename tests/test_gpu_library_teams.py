"""k_library's side-by-side passes ("teams": up to four consecutive passes of a seq + struct library in ONE launch, each on a
share of the workgroups; lib_run in pfmscan_library_api.hip) at the shortest stream that takes that route.

The route is taken only on long streams, so the stream is generated on the device: records of 3000 positions, as many as the
device's compute-unit count asks for (33.6 M positions on 256 CUs).  Every case that is meant to run in teams asks the library
handle how it ran (Library.last_launches) and FAILS when no launch had teams.  Two references in every case:

  (a) the CPU oracle, one motif at a time, on 32 records copied home (the first, the last, those on work-segment boundaries
      where the workgroup index wraps, the rest at random): inside them the device's hits are the oracle's exactly, float32
      sequence scores bit for bit, structure scores within their rounding-error bound (precision_rules), the joint threshold by
      the oracle-side predicate of test_gpu_library_sum.Scores.hits;
  (b) the same call with PFMSCAN_LIB_SEQUENTIAL=1 -- the route the small tests pin to the oracle: the whole hit list, sorted by
      (position, motif), is identical down to the float32 and float64 bits.

Thresholds are quantiles of the oracle's scores on the sample (a high letters quantile, the middle of the structure scores),
chosen so that the whole stream yields some 10^6 hits; the joint thresholds T differ from pass to pass, so that a team that reads
another team's thresholds changes the hit set of the sampled records (checked on the oracle's side in every such case)."""
import os

import numpy as np
import pytest

from test_gpu_library import _below_max, _clear_of, make_library
from test_gpu_library_sum import Scores, check

pytestmark = pytest.mark.gpu

L = 3000                       # record length; a record and its separator: L + 1 stream positions
SEG = 16384                    # windows per work segment of k_library (segment s -> workgroup s mod grid)
N_SAMPLE = 32
CAP = 12 * 10 ** 6             # slots of the hit arrays: every case stays under 10^7 hits
F32, F64 = np.float32, np.float64


class Big(object):
    """the device-resident stream, its sample at home, and what the cases share: motif pools, the oracle's scores"""

    def __init__(self):
        import torch
        import bench
        from rnascan_amd import _lib, pack
        # a context of its own: its hit buffers grow to these capacities and go with it
        self.torch, self.ctx, self.dev = torch, _lib.Context(0), torch.device("cuda", 0)
        self.n_cu = self.ctx.device_info()["n_cu"]
        stride = L + 1
        self.R = -(-(8 * self.n_cu * SEG + 4 * stride) // stride)
        self.codes, prof32, self.n_pos = bench.make_stream(torch, self.dev, self.R, L, 20250318, foreign=0.002, zero_snap=True)
        self.profile = {F32: prof32, F64: prof32.double()}
        # the sample: record 0, the last one, those holding the segment boundaries where the workgroup index of a full grid of
        # 256 wraps, the last boundary of the stream; the rest at random
        rng = np.random.default_rng(5)
        recs = set([0, self.R - 1, ((self.n_pos - 1) // SEG * SEG) // stride] + [k * SEG // stride for k in (1, 255, 256, 257)])
        rest = rng.permutation(self.R)
        recs = np.array(sorted(recs | set(int(r) for r in rest[~np.isin(rest, list(recs))][:N_SAMPLE - len(recs)])), dtype=np.int64)
        assert recs.size == N_SAMPLE
        self.recs = torch.from_numpy(recs).to(self.dev)
        at = (self.recs[:, None] * stride + torch.arange(stride, device=self.dev)[None, :]).reshape(-1)
        codes = self.codes[at].cpu().numpy()
        offsets, lengths = np.arange(N_SAMPLE, dtype=np.int64) * stride, np.full(N_SAMPLE, L, dtype=np.int64)
        self.sample = {dt: pack.Stream(codes, self.profile[dt][at].cpu().numpy(), offsets, lengths) for dt in (F32, F64)}
        self.share = float(N_SAMPLE * stride) / self.n_pos          # of the stream's positions that lie in the sample
        self._pools, self._scores, self._bound = {}, {}, {}
        torch.cuda.synchronize()

    def pool(self, m, cells):
        """-> (letter tables, structure PSSMs, motifs per pass) of a width: more motifs than any case needs, the pass size as
        a library of them reports it; cells "inf": two -inf cells in every third PSSM"""
        if (m, cells) not in self._pools:
            rng = np.random.default_rng(900 + m + (1 if cells == "inf" else 0))
            T, P = make_library(rng, 600, m)
            if cells == "inf":
                for k in range(2, 600, 3):
                    rows = rng.choice(m, size=2, replace=False)
                    P[k, rows, rng.integers(0, 7, size=2)] = -np.inf
            probe = self.ctx.library(T, P)
            info = probe.info()
            probe.close()
            assert info["passes"] > 1
            self._pools[(m, cells)] = (T, P, info["motifs_per_pass"])
        return self._pools[(m, cells)]

    def scores(self, oracle, m, cells, dtype, n, n_most):
        """the oracle's scores of the first n motifs of a pool on the sample (computed once, for the n_most motifs the largest
        case of this pool and these rows needs)"""
        key = (m, cells, dtype)
        T, P, _ = self.pool(m, cells)
        have = self._scores.get(key)
        if have is None or len(have.sq) < n:
            have = self._scores[key] = Scores(oracle, self.sample[dtype], T[:max(n, n_most)], P[:max(n, n_most)])
        sc = Scores.__new__(Scores)
        sc.oracle, sc.s, sc.T, sc.P = oracle, have.s, have.T[:n], have.P[:n]
        sc.sq, sc.st, sc.sums = have.sq[:n], have.st[:n], have.sums[:n]
        return sc

    def row_bound(self, dtype):
        if dtype not in self._bound:
            from rnascan_amd import _lib
            out = self.torch.full((1,), -1.0, dtype=self.torch.float64, device=self.dev)
            self.torch.cuda.synchronize()
            self.ctx.profile_row_bound_dev(self.codes.data_ptr(), self.profile[dtype].data_ptr(), _lib.PROFILE_F32 if dtype == F32 else _lib.PROFILE_F64,
                                           self.n_pos, out.data_ptr())
            self.ctx.synchronize()
            self._bound[dtype] = float(out.item())
            assert np.isfinite(self._bound[dtype])
        return self._bound[dtype]

    def scan(self, lib, dtype, ts, tt, tj=None, capacity=CAP, n_pos=None, sequential=False):
        """one pfmscan_library_hits_dev / _sum_dev call -> (reported count, hits sorted by (position, motif) as device tensors
        -- None when the count exceeds the capacity --, Library.last_launches())"""
        from rnascan_amd import _lib
        torch, ctx = self.torch, self.ctx
        prof, dt = self.profile[dtype], (_lib.PROFILE_F32 if dtype == F32 else _lib.PROFILE_F64)
        n_pos = self.n_pos if n_pos is None else n_pos
        pos = torch.empty(capacity, dtype=torch.int64, device=self.dev)
        mo = torch.empty(capacity, dtype=torch.int32, device=self.dev)
        sq = torch.empty(capacity, dtype=torch.float32, device=self.dev)
        st = torch.empty(capacity, dtype=torch.float64, device=self.dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=self.dev)
        torch.cuda.synchronize()                     # torch's stream has filled them, the scan runs on the ctx's own
        assert "PFMSCAN_LIB_SEQUENTIAL" not in os.environ
        if sequential:
            os.environ["PFMSCAN_LIB_SEQUENTIAL"] = "1"
        try:
            if tj is None:
                ctx.library_hits_dev(lib, self.codes.data_ptr(), prof.data_ptr(), dt, n_pos, ts, tt, capacity, pos.data_ptr(), mo.data_ptr(),
                                     sq.data_ptr(), st.data_ptr(), cnt.data_ptr())
            else:
                ctx.library_hits_sum_dev(lib, self.codes.data_ptr(), prof.data_ptr(), dt, n_pos, ts, tt, tj, self.row_bound(dtype), capacity,
                                         pos.data_ptr(), mo.data_ptr(), sq.data_ptr(), st.data_ptr(), cnt.data_ptr())
            ctx.synchronize()
        finally:
            if sequential:
                del os.environ["PFMSCAN_LIB_SEQUENTIAL"]
        k = int(cnt.item())
        how = lib.last_launches()
        if k > capacity:
            return k, None, how
        order = torch.argsort(pos[:k] * lib.n + mo[:k].long())
        return k, (pos[:k][order], mo[:k][order], sq[:k][order], st[:k][order]), how

    def in_sample(self, hits):
        """the hits inside the sampled records, at the sample's stream positions, as numpy arrays (still sorted)"""
        torch = self.torch
        pos, mo, sq, st = hits
        rec = pos // (L + 1)
        slot = torch.searchsorted(self.recs, rec).clamp_(max=N_SAMPLE - 1)
        sel = self.recs[slot] == rec
        at = slot[sel] * (L + 1) + pos[sel] % (L + 1)
        return at.cpu().numpy(), mo[sel].cpu().numpy(), sq[sel].cpu().numpy(), st[sel].cpu().numpy()


def assert_same_bits(torch, got, want, what):
    """two sorted hit lists on the device: positions, motifs, float32 bits, float64 bits"""
    assert got[0].numel() == want[0].numel(), "%s: %d hits, the reference has %d" % (what, got[0].numel(), want[0].numel())
    columns = (("positions", got[0], want[0]), ("motifs", got[1], want[1]), ("float32 bits", got[2].view(torch.int32), want[2].view(torch.int32)),
               ("float64 bits", got[3].view(torch.int64), want[3].view(torch.int64)))
    for name, x, y in columns:
        if not torch.equal(x, y):
            i = int(torch.nonzero(x != y)[0])
            raise AssertionError("%s: %s differ, first at hit %d of %d: %r, the reference has %r (position %d)"
                                 % (what, name, i, x.numel(), x[i].item(), y[i].item(), int(want[0][i])))


@pytest.fixture(scope="module")
def big(ctx):
    import torch
    n_cu = ctx.device_info()["n_cu"]
    if n_cu < 16:
        pytest.skip("k_library runs its passes side by side on 16 compute units or more; this device has %d" % n_cu)
    if torch.cuda.mem_get_info()[0] < 8e9:
        pytest.skip("needs 8 GB of free HBM")
    b = Big()
    yield b
    b.ctx.close()
    # the stream, its float64 copy, the oracle's scores.  (No torch.cuda.empty_cache(): the placed-array test of
    # test_gpu_parity.py decides from the free device memory what it expects, and giving torch's cache back moves that.)
    b.__dict__.clear()


def thresholds(sc, big, whole_stream_hits):
    """per-motif thresholds from the oracle's scores on the sample: the structure threshold in the middle of the motif's finite
    structure scores (between two of them), the letters threshold at the quantile that leaves the motif whole_stream_hits[k]
    hits in the whole stream if the sample is typical"""
    n = len(sc.sq)
    want = np.broadcast_to(np.asarray(whole_stream_hits, dtype=np.float64), (n,)) * big.share
    ts, tt = np.empty(n), np.empty(n)
    for k in range(n):
        sq = sc.sq[k].astype(np.float64)
        sq = sq[np.isfinite(sq)]
        st = sc.st[k]
        fin = st[np.isfinite(st) & (np.abs(st) < 1e9)]
        t = _below_max(fin, 0.5)
        near = fin[np.abs(fin - t) < 0.01]                   # (_clear_of sorts what it is given: its neighbours of t are these)
        tt[k] = _clear_of(near if (near <= t).any() and (near > t).any() else fin, t)
        passing = float((st[np.isfinite(sc.sq[k])] > tt[k]).sum())          # windows the structure side lets through
        assert passing > 20 * want[k], "the sample is too small for this hit rate"
        ts[k] = _below_max(sq, 1.0 - want[k] / passing)
    return ts, tt


def joint_thresholds(sc, ts, tt, mpp, rng):
    """T[k]: a quantile of the printed sums of motif k's plain hits in the sample (Scores.sum_quantiles) -- the 0.15 / 0.35 /
    0.55 / 0.75 quantile in the first / second / third / fourth pass of a launch, so every pass has visibly other T"""
    n = len(sc.sq)
    levels = [sc.sum_quantiles(ts, tt, rng, q, q, most=10 ** 9) for q in (0.15, 0.35, 0.55, 0.75)]
    return np.array([levels[(k // mpp) % 4][k] for k in range(n)])


# name: (width, rows, PSSM cells, motifs from the pass size, joint threshold, launches, team launches, most teams in a launch)
CASES = {
    "two teams, the second with one motif": (12, F32, "finite", lambda mpp: mpp + 1, False, 1, 1, 2),
    "three teams, -inf cells": (12, F32, "inf", lambda mpp: 3 * mpp - 5, False, 1, 1, 3),
    "four teams and a launch of one, float64 rows": (12, F64, "finite", lambda mpp: 4 * mpp + mpp // 2, False, 2, 1, 4),
    "four teams and two, joint": (12, F32, "finite", lambda mpp: 5 * mpp + 3, True, 2, 2, 4),
    "three teams, float64 rows, joint": (12, F64, "finite", lambda mpp: 2 * mpp + 1, True, 1, 1, 3),
    "16-bit credits": (18, F32, "finite", lambda mpp: 2 * mpp + 3, False, 1, 1, 3),
    "16-bit credits, joint": (18, F32, "finite", lambda mpp: 2 * mpp + 3, True, 1, 1, 3),
    "wide bucket": (40, F32, "finite", lambda mpp: mpp + 2, False, 1, 1, 2),
}


def _case(big, oracle, m, dtype, cells, n_of):
    T, P, mpp = big.pool(m, cells)
    n = n_of(mpp)
    assert mpp < n <= T.shape[0]
    most = max(case[3](mpp) for case in CASES.values() if case[:3] == (m, dtype, cells))
    return T[:n], P[:n], mpp, n, big.scores(oracle, m, cells, dtype, n, most)


@pytest.mark.parametrize("name", list(CASES))
def test_teams_equal_the_oracle_and_the_sequential_route(big, oracle, name):
    m, dtype, cells, n_of, joint, n_launches, n_team_launches, max_teams = CASES[name]
    torch = big.torch
    T, P, mpp, n, sc = _case(big, oracle, m, dtype, cells, n_of)
    rng = np.random.default_rng(31 + n)
    ts, tt = thresholds(sc, big, (6e6 if joint else 3e6) / n)
    tj = joint_thresholds(sc, ts, tt, mpp, rng) if joint else None
    want = sc.hits(ts, tt, tj)
    assert len(want[0]) >= 1000, "the oracle finds %d hits in the sample" % len(want[0])
    if joint:
        # what a team would decide with the thresholds of the launch's FIRST pass is another hit set on the oracle's side
        first = (np.arange(n) // mpp) // 4 * 4 * mpp + np.arange(n) % mpp
        moved = first != np.arange(n)
        assert moved.sum() >= n - 2 * mpp and (tj[first][moved] != tj[moved]).all()
        other = sc.hits(ts, tt, tj[first])
        assert not (len(other[0]) == len(want[0]) and np.array_equal(other[0], want[0]) and np.array_equal(other[1], want[1]))
    lib = big.ctx.library(T, P)
    try:
        assert lib.info()["passes"] == -(-n // mpp)
        assert lib.last_launches() == {"n_launches": 0, "n_team_launches": 0, "max_teams": 0}
        k, hits, how = big.scan(lib, dtype, ts, tt, tj)
        print("%s: n_cu %d, n_pos %d, mpp %d, %d motifs, %d hits, %r" % (name, big.n_cu, big.n_pos, mpp, n, k, how))
        assert how["n_team_launches"] >= 1, "no pass ran in teams: this test no longer tests them (%r)" % how
        assert how == {"n_launches": n_launches, "n_team_launches": n_team_launches, "max_teams": max_teams}
        k_seq, hits_seq, how_seq = big.scan(lib, dtype, ts, tt, tj, sequential=True)
        assert how_seq == {"n_launches": -(-n // mpp), "n_team_launches": 0, "max_teams": 1}
        # the reference's own output: 10^6 .. 10^7 hits, some of every motif
        assert 10 ** 6 <= k_seq <= 10 ** 7, k_seq
        assert int(torch.bincount(hits_seq[1].long(), minlength=n).min()) > 0
        check(big.in_sample(hits), want, big.sample[dtype], P, name)
        assert_same_bits(torch, hits, hits_seq, "teams against one pass after the other")
    finally:
        lib.close()


def _three_teams(big, oracle):
    m, dtype, cells, n_of = CASES["three teams, -inf cells"][:4]
    return (dtype,) + _case(big, oracle, m, dtype, cells, n_of)


def test_gate_boundary(big, oracle):
    """one position under the length from which teams run: the passes one after the other, and the same hits as far as the
    prefix reaches"""
    torch = big.torch
    dtype, T, P, mpp, n, sc = _three_teams(big, oracle)
    ts, tt = thresholds(sc, big, 3e6 / n)
    short = 8 * big.n_cu * SEG - 1
    assert short < big.n_pos
    lib = big.ctx.library(T, P)
    try:
        k, hits, how = big.scan(lib, dtype, ts, tt)
        assert how["n_team_launches"] >= 1, how
        k_short, hits_short, how_short = big.scan(lib, dtype, ts, tt, n_pos=short)
        print("gate boundary: %d positions %r, %d positions %r" % (big.n_pos, how, short, how_short))
        assert how_short == {"n_launches": 3, "n_team_launches": 0, "max_teams": 1}
        keep = hits[0] < short - T.shape[1] + 1
        assert 10 ** 6 <= k_short == int(keep.sum()) < k
        assert_same_bits(torch, hits_short, tuple(x[keep] for x in hits), "the prefix against the whole stream's hits inside it")
    finally:
        lib.close()


def test_skewed_passes_and_the_capacity_protocol(big, oracle):
    """the first pass yields ten times the hits of the other two together, and in teams its workgroups are neighbours: they
    fill a third of the 256 shards of the hit buffers.  With room for twice the hits the call either delivers them all or
    says how much room it needs -- and then delivers them.  The same with room for 5/4 of the hits and for exactly the hits:
    there the dense pass's shards overflow in teams (a shard has room for twice an even share; one pass after the other 5/4
    is enough), and the count the call reported used to be capacity + 1, with which the next call was incomplete again"""
    torch = big.torch
    dtype, T, P, mpp, n, sc = _three_teams(big, oracle)
    ts, tt = thresholds(sc, big, np.where(np.arange(n) < mpp, 3e6 / mpp, 5e4 / mpp))
    lib = big.ctx.library(T, P)
    try:
        total, hits_seq, how_seq = big.scan(lib, dtype, ts, tt, sequential=True)
        assert how_seq["n_team_launches"] == 0
        dense = int((hits_seq[1] < mpp).sum())
        assert dense >= 10 * (total - dense) > 0 and total >= 10 ** 6, (dense, total)
        retried = 0
        for capacity in (2 * total, total + total // 4, total):
            k, hits, how = big.scan(lib, dtype, ts, tt, capacity=capacity)
            print("skewed passes: %d hits, %d of them of pass 0; capacity %d: reported %d, %r" % (total, dense, capacity, k, how))
            assert how["n_team_launches"] >= 1, how
            if hits is None:                                 # the count is above the capacity: the room it asks for suffices
                assert k > capacity
                k2, hits, how = big.scan(lib, dtype, ts, tt, capacity=k)
                print("skewed passes: capacity %d: reported %d" % (k, k2))
                assert how["n_team_launches"] >= 1, how
                assert hits is not None, "capacity %d was asked for and is not enough: now %d" % (k, k2)
                k = k2
                retried += 1
            assert k == total
            assert_same_bits(torch, hits, hits_seq, "capacity %d, teams against one pass after the other" % capacity)
            del hits
        assert retried, "no capacity made the call ask for more: the second half of the protocol did not run"
    finally:
        lib.close()


def test_other_library_kinds_report_their_launches(ctx):
    """k_profile_lib and k_library8 libraries have no teams: last_launches counts their launches"""
    rng = np.random.default_rng(8)
    _, P = make_library(rng, 5, 12)
    prof = rng.dirichlet(np.full(7, 0.3), size=4000).astype(np.float32)
    lib = ctx.library(None, P)
    assert lib.last_launches() == {"n_launches": 0, "n_team_launches": 0, "max_teams": 0}
    ctx.library_hits_host(lib, None, prof, None, 0.0)
    assert lib.last_launches() == {"n_launches": 1, "n_team_launches": 0, "max_teams": 1}
    lib.close()
    S = np.full((20, 12, 8), np.nan)
    S[:, :, :7] = rng.normal(-0.5, 2.0, size=(20, 12, 7))
    lib = ctx.library(None, struct_letters=S)
    codes = rng.integers(0, 7, size=4000).astype(np.uint8)
    ctx.library_hits_letters_host(lib, codes, thr_struct=3.0)
    how = lib.last_launches()
    assert how == {"n_launches": lib.info()["passes"], "n_team_launches": 0, "max_teams": 1}
    # a short seq + struct library of several passes: one launch per pass, no teams
    T2, P2 = make_library(rng, 130, 12)
    lib2 = ctx.library(T2, P2)
    ctx.library_hits_host(lib2, rng.integers(0, 4, size=4000).astype(np.uint8), prof, 8.0, 0.0)
    assert lib2.last_launches() == {"n_launches": lib2.info()["passes"], "n_team_launches": 0, "max_teams": 1}
    assert lib2.info()["passes"] > 1
    lib.close()
    lib2.close()
