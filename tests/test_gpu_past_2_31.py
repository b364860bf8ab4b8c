"""The thresholded, joint-threshold, library and two-stream kernels on device-resident streams that cross the three borders at
which an index width matters (every entry point takes an int64 n_pos):

  B1  profile byte offset 2^32: float32 row 153 391 690
  B2  profile element index 2^31: inside float32 row 306 783 378 (elements 2 147 483 646 .. 2 147 483 652)
  B3  stream position 2^31

Three streams, generated on the device as test_gpu_library_teams.py and bench.make_stream do (records of 3000 positions plus a
separator, 0.2 % foreign letters, probability rows with exact zeros):

  elem      102 730 records = 308 292 730 positions, float32 rows (8.6 GB; a float64 copy inside the float64 cases): beyond B1
            and B2 -- 1 509 352 rows lie past the straddling row -- and long enough for k_library's teams on 256 CUs
  pos       2^31 + 1 500 000 positions of sequence codes 0..3 and a second stream of structure-letter codes 0..6: B3, letters only
  pos_prof  the same length with float32 rows (60.2 GB): B3 with a profile; the span behind 2^31 has 92 work segments, fewer
            than 256 CUs, so lib_run runs its passes one by one after the team launch of the first span

One stream is resident at a time: a test class per stream, its fixtures class-scoped (in a whole-suite run some 113 GB of the
card are free when this module starts; three streams, a float64 copy and a staged copy together do not fit beside that).

References.  The CPU oracle on three slices of 1 M positions copied home -- the head, 1 M positions centred on the border (row
306 783 378 of elem, position 2^31 of pos / pos_prof), the tail -- and on elem a fourth, centred on B1: window scores do not
depend on what lies before the window, and only windows wholly inside a slice count.  There the hit set per motif is the oracle's exactly, float32 scores bit for bit, fp64
letter scores bit for bit, structure scores within their rounding-error bound (precision_rules.assert_struct_tight), the joint
threshold by the oracle-side predicates of test_gpu_sum_hits.py / test_gpu_library_sum.py / pairsum_helpers.py.  Every case
asks for more than 100 hits inside the border slice, hits on both sides of the border, and of the whole list: positions unique
per motif and inside the stream, the count returned within the capacity.  Where two routes promise the same bytes their WHOLE
sorted hit lists are compared bit for bit.  Thresholds are order statistics of the oracle's scores on the tail slice, chosen so
that a whole stream stays under the capacity of 2^24 hits.

One window is planted on the last 12 positions before the final separator of every stream -- the best letters of T12 (and of
S12 on the structure-letter stream), one-hot rows on the best cells of P12 -- and every case that scans with that motif asserts
the hit at its 64-bit position.  One row of the last record carries the row sum 1 + 2^-16: the row bound of the profile must be
exactly that, so pfmscan_profile_row_bound_dev has read the far end of the profile.

The two-phase routes run on a context created with PFMSCAN_TWO_PHASE=1: k_struct_at through pfmscan_hits_adaptive_dev, and
k_struct_at_sum -- which no _dev entry point reaches: pfmscan_hits_sum_dev is always one fused pass -- through
pfmscan_hits_sum_staged on a copy of elem staged from the host.  Both must give the positions and float32 bits of the fused
pass over the whole stream."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import assert_f32_bits_equal
from pairsum_helpers import printed_sum
from pairsum_helpers import table as letters_table
from precision_rules import assert_struct_tight
from test_gpu_library import make_library
from test_gpu_library_sum import Scores
from test_gpu_library_sum import check as check_library
from test_gpu_library_teams import assert_same_bits
from test_gpu_parity import rand_struct_pssm, rand_table
from test_gpu_sum_hits import want_sum_of

pytestmark = pytest.mark.gpu

L = 3000                       # record length; a record and its separator: STRIDE stream positions
STRIDE = L + 1
SLICE = 1000000                # positions per slice copied home
CAP = 1 << 24                  # slots of the hit arrays
R_ELEM = 102730                # records of `elem`
ROW_B1 = 153391690             # float32 rows: byte offset 2^32
ROW_B2 = 306783378             # float32 rows: the row that holds element 2^31
N_POS = (1 << 31) + 1500000    # `pos` and `pos_prof` (N_POS of test_gpu_big_streams.py)
F32, F64 = np.float32, np.float64


def _make_motifs():
    rng = np.random.default_rng(20261019)
    mo = SimpleNamespace()
    mo.T12, mo.P12 = rand_table(rng, 12), rand_struct_pssm(rng, 12)
    mo.T24, mo.P24 = rand_table(rng, 24), rand_struct_pssm(rng, 24)
    mo.T200, mo.P200 = rand_table(rng, 200), rand_struct_pssm(rng, 200)
    mo.LT, mo.LP = make_library(rng, 97, 12)                   # two passes of k_library at w = 12 (96 motifs per pass)
    mo.LT[0], mo.LP[0] = mo.T12, mo.P12
    mo.SP = np.stack([rand_struct_pssm(rng, 12) for _ in range(16)])      # k_profile_lib
    mo.SP[0] = mo.P12
    mo.S12, mo.T40, mo.S40 = letters_table(rng, 12, 7), rand_table(rng, 40), letters_table(rng, 40, 7)
    mo.T100 = rand_table(rng, 100)
    mo.L8 = np.stack([letters_table(rng, 12, 7) for _ in range(20)])      # k_library8
    mo.L8[0] = mo.S12
    mo.PT = np.stack([rand_table(rng, 12) for _ in range(20)])             # the two-FASTA library
    mo.PS = np.stack([letters_table(rng, 12, 7) for _ in range(20)])
    mo.PT[0], mo.PS[0] = mo.T12, mo.S12
    return mo


MO = _make_motifs()
SINGLE = {"w12": (MO.T12, MO.P12), "w24": (MO.T24, MO.P24), "w200": (MO.T200, MO.P200)}


def _best(table, n_letters):
    return np.argmax(np.where(np.isfinite(table[:, :n_letters]), table[:, :n_letters], -1e300), axis=1)


def _need(torch, gb, what):
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < gb * 1e9:
        pytest.skip("%s needs %d GB of free HBM, %.1f GB are free" % (what, gb, free / 1e9))


class Box(object):
    """a device-resident stream, its slices at home, and what its cases share"""

    def __init__(self, name, torch, codes, n_pos, centre, profile=None, codes2=None, also=()):
        self.name, self.torch, self.dev = name, torch, codes.device
        self.codes, self.codes2, self.profile, self.n_pos, self.centre = codes, codes2, profile, n_pos, centre
        end = n_pos - 1                                             # the final separator
        codes[end] = 7
        codes[end - 12:end] = torch.from_numpy(_best(MO.T12, 4).astype(np.uint8)).to(self.dev)
        if codes2 is not None:
            codes2[end] = 7
            codes2[end - 12:end] = torch.from_numpy(_best(MO.S12, 7).astype(np.uint8)).to(self.dev)
        if profile is not None:
            profile[end] = 0
            rows = np.zeros((12, 7), dtype=np.float32)
            rows[np.arange(12), _best(MO.P12, 7)] = 1.0
            profile[end - 12:end] = torch.from_numpy(rows).to(self.dev)
            self.far_row = end - 2000                               # a row of the last record with the largest sum of the stream
            codes[self.far_row] = 0
            profile[self.far_row] = torch.tensor([0.5, 0.5, 2.0 ** -16, 0, 0, 0, 0], dtype=torch.float32, device=self.dev)
        self.planted = end - 12
        # slices: the head, the border, the tail (the thresholds come from it), then any further border
        self.lo = (0, centre - SLICE // 2, n_pos - SLICE) + tuple(c - SLICE // 2 for c in also)
        assert self.lo[1] >= SLICE and self.lo[1] + SLICE <= self.lo[2] and all(SLICE <= lo <= self.lo[1] - SLICE for lo in self.lo[3:])
        self.borders = [(1, centre)] + [(3 + j, c) for j, c in enumerate(also)]
        self.home = []
        for lo in self.lo:
            h = SimpleNamespace(lo=lo, codes=codes[lo:lo + SLICE].cpu().numpy(), codes2=None, profile=None)
            if codes2 is not None:
                h.codes2 = codes2[lo:lo + SLICE].cpu().numpy()
            if profile is not None:
                h.profile = profile[lo:lo + SLICE].cpu().numpy()
            self.home.append(h)
        self.out = SimpleNamespace(pos=torch.empty(CAP, dtype=torch.int64, device=self.dev), mo=torch.empty(CAP, dtype=torch.int32, device=self.dev),
                                   sq=torch.empty(CAP, dtype=torch.float32, device=self.dev), st=torch.empty(CAP, dtype=torch.float64, device=self.dev),
                                   cnt=torch.zeros(1, dtype=torch.int64, device=self.dev))
        self.cache = {}
        torch.cuda.synchronize()

    def rows(self, i, dtype):
        """the profile rows of slice i as the rows of that dtype hold them"""
        return self.home[i].profile if dtype == F32 else self.home[i].profile.astype(F64)

    def close(self):
        self.__dict__.clear()


class Rows64(object):
    """a float64 copy of a stream's rows, made and freed inside a case"""

    def __init__(self, box):
        self.box = box

    def __enter__(self):
        _need(self.box.torch, 32, "the float64 copy of the rows")
        self.rows = self.box.profile.double()
        self.box.torch.cuda.synchronize()
        return self.rows

    def __exit__(self, *exc):
        del self.rows
        self.box.torch.cuda.empty_cache()


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device that has faulted runs nothing more of this module: the session ends instead of launching the next case"""
    import torch
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                               # noqa: BLE001 (whatever the runtime raises: the device is not usable)
        pytest.exit("the device reports an error after this case, nothing more is launched: %s" % e, returncode=3)


def _context(two_phase):
    from rnascan_amd import _lib
    assert "PFMSCAN_TWO_PHASE" not in os.environ
    os.environ["PFMSCAN_TWO_PHASE"] = str(two_phase)         # read when the context is created
    try:
        return _lib.Context(0)
    finally:
        del os.environ["PFMSCAN_TWO_PHASE"]


@pytest.fixture(scope="module")
def own():
    """contexts of this module's own (their hit buffers grow to 2^24 hits and go with them): one per forced route"""
    import torch
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    print("past 2^31: %.1f GB of %.1f GB of HBM free at module start" % (free / 1e9, total / 1e9))
    c = SimpleNamespace(fused=_context(0), two_phase=_context(1))
    c.n_cu = c.fused.device_info()["n_cu"]
    yield c
    c.fused.close()
    c.two_phase.close()
    torch.cuda.empty_cache()


def _with_profile(torch, name, records, n_pos, centre, seed, also=()):
    import bench
    dev = torch.device("cuda", 0)
    codes, profile, n_made = bench.make_stream(torch, dev, records, L, seed, foreign=0.002, zero_snap=True)
    assert n_made >= n_pos and n_made - n_pos < STRIDE
    box = Box(name, torch, codes, n_pos, centre, profile=profile, also=also)
    print("past 2^31: stream %s: %d positions, %.2f GB of codes, %.1f GB of float32 rows" % (name, n_pos, n_pos / 1e9, n_pos * 28 / 1e9))
    return box


@pytest.fixture(scope="class")
def elem(own):
    import torch
    _need(torch, 12, "the stream beyond 2^31 profile elements")
    box = _with_profile(torch, "elem", R_ELEM, R_ELEM * STRIDE, ROW_B2, 20261019, also=(ROW_B1,))       # a fourth slice: centred on B1
    assert box.n_pos * 7 > (1 << 31) + 7 * 10 ** 6 and box.n_pos >= 8 * own.n_cu * 16384
    yield box
    box.close()
    torch.cuda.empty_cache()


@pytest.fixture(scope="class")
def pos_prof(own):
    import torch
    _need(torch, 80, "the stream beyond 2^31 positions with a profile")
    box = _with_profile(torch, "pos_prof", -(-N_POS // STRIDE), N_POS, 1 << 31, 20261020)
    yield box
    box.close()
    torch.cuda.empty_cache()


@pytest.fixture(scope="class")
def pos(own):
    import torch
    _need(torch, 8, "the two letter streams beyond 2^31 positions")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(20261021)
    codes = torch.randint(0, 4, (N_POS,), dtype=torch.uint8, device=dev, generator=g)
    codes2 = torch.randint(0, 7, (N_POS,), dtype=torch.uint8, device=dev, generator=g)
    chunk = 1 << 28
    for c in (codes, codes2):
        for lo in range(0, N_POS, chunk):                           # foreign letters, on either side
            part = c[lo:min(N_POS, lo + chunk)]
            part[torch.rand(part.numel(), device=dev, generator=g) < 0.002] = 7
        c[L::STRIDE] = 7                                            # separators: records of 3000
    box = Box("pos", torch, codes, N_POS, 1 << 31, codes2=codes2)
    print("past 2^31: stream pos: %d positions, two code streams of %.2f GB" % (N_POS, N_POS / 1e9))
    yield box
    box.close()
    torch.cuda.empty_cache()


# ---- order statistics for thresholds ----------------------------------------------------------------------------------------
def _usable(v):
    v = np.asarray(v, dtype=np.float64)
    return v[np.isfinite(v) & (np.abs(v) < 1e9)]


def _between_top(values, k):
    """a threshold that exactly k of the values exceed: the middle of the gap under the k-th largest"""
    v = _usable(values)
    assert v.size > k + 1
    top = np.sort(np.partition(v, v.size - k - 1)[v.size - k - 1:])        # the k + 1 largest, ascending
    assert top[0] < top[1], "a tie at the threshold"
    return float(top[0] + (top[1] - top[0]) / 2)


def _kth_below(values, k):
    """the (k + 1)-th largest value: `>` leaves the k largest (float32 scores compare exactly)"""
    v = _usable(values)
    assert v.size > k + 1
    return float(np.partition(v, v.size - k - 1)[v.size - k - 1])


def _seq_struct_thresholds(sq, st, want):
    """the structure threshold in the middle of the structure scores, the letters threshold so that about `want` windows pass both"""
    tt = _between_top(st[::8], _usable(st[::8]).size // 2)
    ok = np.isfinite(sq)
    with np.errstate(invalid="ignore"):
        passing = int((st[ok] > tt).sum())
    ts = _kth_below(sq[ok], int(round(want * float(ok.sum()) / passing)))
    return ts, tt


def _mid(values):
    """a joint threshold that half of the values exceed, between two of them"""
    v = np.sort(_usable(values))
    assert v.size >= 4
    return float(v[v.size // 2 - 1] + (v[v.size // 2] - v[v.size // 2 - 1]) / 2)


# ---- the whole list and the slices --------------------------------------------------------------------------------------------
def _collect(box, n_motifs=None):
    """the call's output as sorted device tensors (copies): (pos, seq, struct) by position, or (pos, motif, seq, struct) by
    (position, motif); the whole-list invariants"""
    torch, o = box.torch, box.out
    k = int(o.cnt.item())
    assert 0 < k <= CAP, "%d hits reported, the capacity is %d" % (k, CAP)
    key = o.pos[:k] if n_motifs is None else o.pos[:k] * n_motifs + o.mo[:k].long()
    key, order = torch.sort(key)
    assert bool((key[1:] > key[:-1]).all()), "a position is reported twice for one motif"
    pos = o.pos[:k][order]
    if n_motifs is not None:
        mo = o.mo[:k][order]
        assert int(mo.min()) >= 0 and int(mo.max()) < n_motifs
        return pos, mo, o.sq[:k][order], o.st[:k][order]
    return pos, o.sq[:k][order], o.st[:k][order]


def _inside(box, hits, m):
    assert int(hits[0][0]) >= 0 and int(hits[0].max()) <= box.n_pos - m, "a hit outside [0, n_pos - m]"


def _in_slice(box, i, hits, m):
    """the hits whose windows lie wholly inside slice i, positions relative to the slice, as numpy arrays (still sorted)"""
    lo = box.lo[i]
    sel = (hits[0] >= lo) & (hits[0] <= lo + SLICE - m)
    return (hits[0][sel].cpu().numpy() - lo,) + tuple(x[sel].cpu().numpy() for x in hits[1:])


def _border(box, hits, m, what):
    """more than 100 hits inside every border slice, on both sides of the border"""
    for i, centre in box.borders:
        p = _in_slice(box, i, hits, m)[0] + box.lo[i]
        below, above = int((p < centre).sum()), int((p >= centre).sum())
        print("past 2^31: %s on %s: %d hits in the stream, %d in the border slice: %d below %d, %d at or above it"
              % (what, box.name, hits[0].numel(), p.size, below, centre, above))
        assert p.size > 100 and below > 0 and above > 0, (what, centre, p.size, below, above)


def _zero(box):
    box.out.cnt.zero_()
    box.torch.cuda.synchronize()                     # torch's stream has zeroed the counter, the scan runs on the context's own


# ---- single motifs: k_profile_fixed / k_profile / k_wide with HITS and SUM, k_struct_at ------------------------------------
def _single_scores(oracle, box, name, parts, dtype, i):
    key = ("single", name, parts, dtype, i)
    if key not in box.cache:
        T, P = SINGLE[name]
        sq = oracle.stream_seq(box.home[i].codes, T) if "seq" in parts else None
        box.cache[key] = (sq, oracle.stream_struct(box.rows(i, dtype), P))
    return box.cache[key]


def _single_want(oracle, sq, st, m, ts, tt, tj):
    p = oracle.stream_hits(sq, st, ts, tt)
    p = p[p <= SLICE - m]
    if tj is not None:
        with np.errstate(invalid="ignore"):
            p = p[want_sum_of(sq[p], st[p]) > tj]
    return p


def _single_scan(box, ctx, motif, rows, dtype, ts, tt, tj=None, adaptive=False):
    from rnascan_amd import _lib
    o, dt = box.out, (_lib.PROFILE_F32 if dtype == F32 else _lib.PROFILE_F64)
    codes = box.codes.data_ptr() if motif.has_letters else None
    sq = o.sq.data_ptr() if motif.has_letters else None
    _zero(box)
    if tj is not None:
        ctx.hits_sum_dev(motif, codes, rows.data_ptr(), dt, box.n_pos, ts, tt, tj, CAP, o.pos.data_ptr(), sq, o.st.data_ptr(), o.cnt.data_ptr())
    elif adaptive:
        ctx.hits_adaptive_dev(motif, codes, rows.data_ptr(), dt, box.n_pos, ts, tt, CAP, o.pos.data_ptr(), sq, o.st.data_ptr(), o.cnt.data_ptr())
    else:
        ctx.hits_dev(motif, codes, rows.data_ptr(), dt, box.n_pos, ts, tt, CAP, o.pos.data_ptr(), sq, o.st.data_ptr(), o.cnt.data_ptr())
    ctx.synchronize()
    return _collect(box)


# case: (motif, its parts, rows, route, per-slice hits asked for)
SINGLE_CASES = {
    "fused w12 (k_profile_fixed)": ("w12", "seq+struct", F32, "hits", 500),
    "fused w24 (k_profile)": ("w24", "seq+struct", F32, "hits", 500),
    "fused w12, structure only": ("w12", "struct", F32, "hits", 500),
    "fused w24, structure only": ("w24", "struct", F32, "hits", 500),
    "fused w12, float64 rows": ("w12", "seq+struct", F64, "hits", 500),
    "two-phase w12 (k_struct_at)": ("w12", "seq+struct", F32, "adaptive", 500),
    "joint w12 (k_profile_fixed_sum)": ("w12", "seq+struct", F32, "sum", 600),
    "joint w24 (k_profile_sum)": ("w24", "seq+struct", F32, "sum", 600),
    "joint two-phase w12 (k_struct_at_sum), staged copy": ("w12", "seq+struct", F32, "staged sum", 600),
    "w200 (k_wide)": ("w200", "seq+struct", F32, "hits", 200),
    "joint w200 (k_wide_sum)": ("w200", "seq+struct", F32, "sum", 300),
}


def _single_case(own, oracle, box, case):
    name, parts, dtype, route, want = SINGLE_CASES[case]
    T, P = SINGLE[name]
    m = P.shape[0]
    sq, st = _single_scores(oracle, box, name, parts, dtype, 2)           # thresholds: from the tail slice
    if sq is None:
        ts, tt = -np.inf, _between_top(st, want)
    else:
        ts, tt = _seq_struct_thresholds(sq, st, want)
    tj = None
    if route.endswith("sum"):
        plain = oracle.stream_hits(sq, st, ts, tt)
        tj = _mid(want_sum_of(sq[plain], st[plain]))
    two_phase = route in ("adaptive", "staged sum")
    ctx = own.two_phase if two_phase else own.fused
    motif = ctx.motif(T if sq is not None else None, P)
    try:
        if route == "staged sum":
            # the stream once more, staged from the host (the only form that takes two passes under a joint threshold)
            _need(box.torch, 10, "a staged copy of the stream")
            staging = _context(1)                          # the staged copy goes with this context
            try:
                staged_motif = staging.motif(T, P)
                staging.stage(box.codes.cpu().numpy(), box.profile.cpu().numpy())
                got = staging.hits_sum_staged(staged_motif, ts, tt, tj, capacity=CAP)
                staged_motif.close()
            finally:
                staging.close()
            assert 0 < got[0].size <= CAP and (np.diff(got[0]) > 0).all()
            hits = tuple(box.torch.from_numpy(x).to(box.dev) for x in got)
        elif dtype == F64:
            with Rows64(box) as rows:
                hits = _single_scan(box, ctx, motif, rows, dtype, ts, tt, tj)
        else:
            hits = _single_scan(box, ctx, motif, box.profile, dtype, ts, tt, tj, adaptive=(route == "adaptive"))
    finally:
        motif.close()
    _inside(box, hits, m)
    for i in range(len(box.lo)):
        wsq, wst = _single_scores(oracle, box, name, parts, dtype, i)
        wp = _single_want(oracle, wsq, wst, m, ts, tt, tj)
        gp, gq, gt = _in_slice(box, i, hits, m)
        assert np.array_equal(gp, wp), "%s, slice at %d: %d hits, the oracle has %d" % (case, box.lo[i], gp.size, wp.size)
        if wsq is not None:
            assert_f32_bits_equal(gq, wsq[wp])
        assert_struct_tight(gt, box.rows(i, dtype), P, positions=wp)
        if tj is not None:
            assert wp.size < _single_want(oracle, wsq, wst, m, ts, tt, None).size, "the joint threshold drops nothing here"
    _border(box, hits, m, case)
    if name == "w12":
        assert bool((hits[0] == box.planted).any()), "the window planted at %d is not among the hits" % box.planted
    if two_phase:
        # the same positions and float32 bits as the fused pass, over the whole stream
        motif = own.fused.motif(T, P)
        try:
            fused = _single_scan(box, own.fused, motif, box.profile, dtype, ts, tt, tj)
        finally:
            motif.close()
        torch = box.torch
        assert hits[0].numel() == fused[0].numel() and torch.equal(hits[0], fused[0])
        assert torch.equal(hits[1].view(torch.int32), fused[1].view(torch.int32))


# ---- k_library: teams, the short last span, the joint threshold, the row bound ------------------------------------------------
def _row_bound_torch(box):
    """pfmscan_profile_row_bound restated on the device: the columns added in fp64, c ascending, over chunks; the largest sum
    over the rows whose code is not 7"""
    torch = box.torch
    best = torch.zeros((), dtype=torch.float64, device=box.dev)
    chunk = 1 << 24
    for lo in range(0, box.n_pos, chunk):
        hi = min(box.n_pos, lo + chunk)
        r = box.profile[lo:hi]
        s = r[:, 0].double()
        for c in range(1, 7):
            s = s + r[:, c].double()
        s = s[(box.codes[lo:hi] & 7) != 7]
        if s.numel():
            best = torch.maximum(best, s.max())
    return float(best.item())


class LibState(object):
    """what the library cases of one stream share: per-motif thresholds from the tail slice, the motifs checked against the
    oracle and their scores on the three slices, the row bound, the plain hit list"""

    def __init__(self, own, oracle, box):
        self.own, self.oracle, self.box = own, oracle, box
        tail = box.home[2]
        n = MO.LT.shape[0]
        self.ts, self.ts_joint, self.tt, self.tj = np.empty(n), np.empty(n), np.empty(n), np.empty(n)
        for k in range(n):                                     # about 30 hits per motif and 1 M positions: 3 x 10^-5
            sq, st = oracle.stream_seq(tail.codes, MO.LT[k]), oracle.stream_struct(tail.profile, MO.LP[k])
            self.ts[k], self.tt[k] = _seq_struct_thresholds(sq, st, 30)
            self.ts_joint[k] = _seq_struct_thresholds(sq, st, 60)[0]
            plain = oracle.stream_hits(sq, st, self.ts_joint[k], self.tt[k])
            self.tj[k] = _mid(want_sum_of(sq[plain], st[plain]))
        probe = own.fused.library(MO.LT, MO.LP)
        info = probe.info()
        probe.close()
        self.mpp = info["motifs_per_pass"]
        assert info["passes"] == 2 and self.mpp < n
        rng = np.random.default_rng(8)
        ends = {0, self.mpp - 1, self.mpp, n - 1}              # the first and the last motif of each pass
        rest = [int(k) for k in rng.permutation(n) if int(k) not in ends][:8 - len(ends)]
        self.sel = np.array(sorted(ends | set(rest)))
        assert self.sel.size == 8
        self._scores, self._bound, self._plain = {}, None, None

    def scores(self, i, dtype):
        if (i, dtype) not in self._scores:
            s = SimpleNamespace(codes=self.box.home[i].codes, profile=self.box.rows(i, dtype))
            self._scores[(i, dtype)] = Scores(self.oracle, s, MO.LT[self.sel], MO.LP[self.sel])
        return self._scores[(i, dtype)]

    def row_bound(self):
        if self._bound is None:
            from rnascan_amd import _lib
            box, ctx = self.box, self.own.fused
            out = box.torch.full((1,), -1.0, dtype=box.torch.float64, device=box.dev)
            box.torch.cuda.synchronize()
            ctx.profile_row_bound_dev(box.codes.data_ptr(), box.profile.data_ptr(), _lib.PROFILE_F32, box.n_pos, out.data_ptr())
            ctx.synchronize()
            self._bound = float(out.item())
        return self._bound

    def scan(self, lib, rows, dtype, joint, sequential=False):
        from rnascan_amd import _lib
        box, ctx, o = self.box, self.own.fused, self.box.out
        dt = _lib.PROFILE_F32 if dtype == F32 else _lib.PROFILE_F64
        _zero(box)
        assert "PFMSCAN_LIB_SEQUENTIAL" not in os.environ
        if sequential:
            os.environ["PFMSCAN_LIB_SEQUENTIAL"] = "1"
        try:
            if joint:
                ctx.library_hits_sum_dev(lib, box.codes.data_ptr(), rows.data_ptr(), dt, box.n_pos, self.ts_joint, self.tt, self.tj, self.row_bound(),
                                         CAP, o.pos.data_ptr(), o.mo.data_ptr(), o.sq.data_ptr(), o.st.data_ptr(), o.cnt.data_ptr())
            else:
                ctx.library_hits_dev(lib, box.codes.data_ptr(), rows.data_ptr(), dt, box.n_pos, self.ts, self.tt, CAP, o.pos.data_ptr(),
                                     o.mo.data_ptr(), o.sq.data_ptr(), o.st.data_ptr(), o.cnt.data_ptr())
            ctx.synchronize()
        finally:
            if sequential:
                del os.environ["PFMSCAN_LIB_SEQUENTIAL"]
        return _collect(box, lib.n), lib.last_launches()

    def plain_hits(self):
        """the float32 plain hit list in teams (cases 5 and 13; the site sums of case 8 start from it)"""
        if self._plain is None:
            lib = self.own.fused.library(MO.LT, MO.LP)
            try:
                self._plain = self.scan(lib, self.box.profile, F32, False)
            finally:
                lib.close()
        return self._plain

    def check(self, hits, dtype, joint, what):
        """the hits of the eight checked motifs inside the three slices against the oracle"""
        box, torch = self.box, self.box.torch
        slot = torch.full((MO.LT.shape[0],), -1, dtype=torch.int64, device=box.dev)
        slot[torch.from_numpy(self.sel).to(box.dev)] = torch.arange(8, device=box.dev)
        keep = slot[hits[1].long()] >= 0
        mine = (hits[0][keep], slot[hits[1].long()][keep].int(), hits[2][keep], hits[3][keep])       # still sorted: sel ascends
        ts, tt = (self.ts_joint if joint else self.ts)[self.sel], self.tt[self.sel]
        for i in range(len(box.lo)):
            sc = self.scores(i, dtype)
            want = sc.hits(ts, tt, self.tj[self.sel] if joint else None)
            fits = want[0] <= SLICE - 12
            want = tuple(x[fits] for x in want)
            check_library(_in_slice(box, i, mine, 12), want, sc.s, MO.LP[self.sel], "%s, slice at %d" % (what, box.lo[i]))
            if joint:
                assert len(want[0]) < int((sc.hits(ts, tt)[0] <= SLICE - 12).sum()), "the joint threshold drops nothing here"
        _border(box, mine, 12, what + ", the 8 motifs checked")
        assert bool(((hits[0] == box.planted) & (hits[1] == 0)).any()), "motif 0's window planted at %d is not among the hits" % box.planted


@pytest.fixture(scope="class")
def lib_elem(own, oracle, elem):
    state = LibState(own, oracle, elem)
    yield state
    state.__dict__.clear()


@pytest.fixture(scope="class")
def lib_prof(own, oracle, pos_prof):
    state = LibState(own, oracle, pos_prof)
    yield state
    state.__dict__.clear()


def _library_case(state, kind, teams_want, sequential_want):
    box, torch = state.box, state.box.torch
    dtype, joint = (F64 if "float64" in kind else F32), kind.startswith("joint")
    what = "library of 97, %s" % kind
    if joint:
        bound = state.row_bound()
        assert bound == 1.0 + 2.0 ** -16, "the row bound %r is not the sum of the row planted at %d" % (bound, box.far_row)
        restated = _row_bound_torch(box)
        assert np.float64(bound).view(np.uint64) == np.float64(restated).view(np.uint64), (bound, restated)
    lib = state.own.fused.library(MO.LT, MO.LP)
    try:
        if dtype == F64:
            with Rows64(box) as rows:
                hits, how = state.scan(lib, rows, dtype, joint)
                hits_seq, how_seq = state.scan(lib, rows, dtype, joint, sequential=True)
        else:
            hits, how = state.plain_hits() if kind == "plain" else state.scan(lib, box.profile, dtype, joint)
            hits_seq, how_seq = state.scan(lib, box.profile, dtype, joint, sequential=True)
    finally:
        lib.close()
    print("past 2^31: %s on %s: %d hits, %r; one pass after the other: %r" % (what, box.name, hits[0].numel(), how, how_seq))
    assert how["n_team_launches"] >= 1, "no pass ran in teams: this test no longer tests them (%r)" % how
    assert how == teams_want and how_seq == sequential_want, (how, how_seq)
    _inside(box, hits, 12)
    assert int(torch.bincount(hits[1].long(), minlength=97).min()) > 0
    state.check(hits, dtype, joint, what)
    assert_same_bits(torch, hits, hits_seq, what + ": teams against one pass after the other")


# ---- k_profile_lib ----------------------------------------------------------------------------------------------------------------
def _struct_library_case(own, oracle, box, dtype):
    from rnascan_amd import _lib
    n, what = MO.SP.shape[0], "structure-only library of 16, %s rows" % np.dtype(dtype).name
    key = ("proflib", dtype)
    if key not in box.cache:
        box.cache[key] = [[oracle.stream_struct(box.rows(i, dtype), MO.SP[k]) for k in range(n)] for i in range(len(box.lo))]
    full = box.cache[key]
    thr = np.array([_between_top(full[2][k], 30) for k in range(n)])
    lib = own.fused.library(None, MO.SP)
    o, dt = box.out, (_lib.PROFILE_F32 if dtype == F32 else _lib.PROFILE_F64)

    def scan(rows):
        _zero(box)
        own.fused.library_hits_dev(lib, None, rows.data_ptr(), dt, box.n_pos, None, thr, CAP, o.pos.data_ptr(), o.mo.data_ptr(), o.sq.data_ptr(),
                                   o.st.data_ptr(), o.cnt.data_ptr())
        own.fused.synchronize()
        return _collect(box, n)
    try:
        if dtype == F64:
            with Rows64(box) as rows:
                hits = scan(rows)
        else:
            hits = scan(box.profile)
        assert lib.last_launches() == {"n_launches": 1, "n_team_launches": 0, "max_teams": 1}
    finally:
        lib.close()
    _inside(box, hits, 12)
    for i in range(len(box.lo)):
        gp, gm, _, gt = _in_slice(box, i, hits, 12)
        for k in range(n):
            wp = oracle.stream_hits(None, full[i][k], -np.inf, thr[k])
            wp = wp[wp <= SLICE - 12]
            sel = gm == k
            assert np.array_equal(gp[sel], wp), "%s, motif %d, slice at %d: %d hits, the oracle has %d" % (what, k, box.lo[i], int(sel.sum()), wp.size)
            assert_struct_tight(gt[sel], box.rows(i, dtype), MO.SP[k], positions=wp)
    _border(box, hits, 12, what)


# ---- k_site_sums_lib ----------------------------------------------------------------------------------------------------------
def _site_sums_case(lib_elem):
    """pfmscan_site_sums_lib_dev under the library's hits in the records wholly inside the border and tail slices, against the
    same call on those records copied into a small stream, positions shifted: the accumulators are order-free integers, and
    the small-stream call is tied to the rules by test_gpu_sites_lib.py"""
    from rnascan_amd import _lib
    box, torch, ctx = lib_elem.box, lib_elem.box.torch, lib_elem.own.fused
    hits, _ = lib_elem.plain_hits()
    n, m = MO.LT.shape[0], 12
    rec = hits[0] // STRIDE
    keep = torch.zeros_like(rec, dtype=torch.bool)
    recs = []
    for i in (1, 2):
        first, last = -(-box.lo[i] // STRIDE), (box.lo[i] + SLICE) // STRIDE - 1        # records wholly inside the slice
        keep |= (rec >= first) & (rec <= last)
        recs.append(torch.arange(first, last + 1, device=box.dev))
    recs = torch.cat(recs)
    pos, mot = hits[0][keep].cpu().numpy(), hits[1][keep].cpu().numpy()
    assert pos.size > 1000 and (pos < ROW_B2).any() and (pos > ROW_B2).any() and np.unique(mot).size == n
    order = _lib.site_order_lib(pos, mot, n)                                            # motif-major
    pos, mot = pos[order], mot[order]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(box.dev)                # noqa: E731

    def sums(codes, profile, n_pos, positions, offsets):
        lengths = np.full(offsets.size, L, dtype=np.int64)
        gf, gr, gm = _lib.site_groups_lib(positions, mot, n, offsets, lengths, m)
        acc = torch.full((n, _lib.SITE_LIMBS, m * 7), -1, dtype=torch.int64, device=box.dev)         # the call zeroes them itself
        counts = torch.full((n, m, 8), -1, dtype=torch.int64, device=box.dev)
        d = [up(x) for x in (positions, gf, gr, gm, offsets, lengths)]
        torch.cuda.synchronize()
        ctx.site_sums_lib_dev(codes, profile, F32, n_pos, d[0], positions.size, d[1], d[2], d[3], gr.size, d[4], d[5], offsets.size, n, m, 0, acc, counts)
        ctx.synchronize()
        raw = acc.cpu().numpy().view(np.uint64)
        return _lib.site_acc_add(np.zeros_like(raw), raw), counts.cpu().numpy().view(np.uint64), gr.size

    big = sums(box.codes, box.profile, box.n_pos, pos, np.arange(R_ELEM, dtype=np.int64) * STRIDE)
    at = (recs[:, None] * STRIDE + torch.arange(STRIDE, device=box.dev)[None, :]).reshape(-1)
    codes, profile = box.codes[at].contiguous(), box.profile[at].contiguous()
    slot = np.searchsorted(recs.cpu().numpy(), pos // STRIDE)
    small = sums(codes, profile, at.numel(), slot * STRIDE + pos % STRIDE, np.arange(recs.numel(), dtype=np.int64) * STRIDE)
    print("past 2^31: library site sums on elem: %d hits in %d groups under %d records" % (pos.size, big[2], recs.numel()))
    assert big[2] == small[2]
    assert np.array_equal(big[0], small[0]), "the accumulators differ, first at %r" % (np.argwhere(big[0] != small[0])[:1],)
    assert np.array_equal(big[1], small[1])
    assert int(big[1].sum()) == pos.size * m and big[0].any()


# ---- the letter kernels on `pos` --------------------------------------------------------------------------------------------------
def _letters_scores(oracle, box, which, table, tag, i):
    key = ("letters", which, tag, i)
    if key not in box.cache:
        h = box.home[i]
        box.cache[key] = oracle.stream_seq(h.codes, table) if which == "seq" else oracle.stream_letters_f64(h.codes2, table)
    return box.cache[key]


def _pair_want(oracle, sq, st, m, t1, t2, T):
    """pairsum_helpers.pair_sum_hits, the printed sums taken only where the unrounded sum comes within 0.01 of T (a printed
    column differs from its score by at most 0.0005)"""
    p = oracle.stream_hits(sq, st, t1, t2)
    p = p[p <= SLICE - m]
    if T is None:
        return p
    p = p[sq[p].astype(F64) + st[p] > T - 0.01]
    return p[printed_sum(sq[p], st[p]) > T]


# case: (width, thr_seq finite, joint, the route pair_sum_route must report)
PAIR_CASES = {
    "plain, finite -m (k_letters_cred<PAIR>)": (12, True, False, "NONE"),
    "joint, finite -m (k_letters_cred<PAIR, SUM>)": (12, True, True, "FUSED"),
    "joint, -m -inf (k_pair_cred_sum)": (12, False, True, "CREDITS"),
    "joint, w40, -m -inf (k_pair_sum_dense)": (40, False, True, "DENSE"),
}


def _pair_case(own, oracle, pos, case):
    from rnascan_amd import _lib
    m, finite, joint, route = PAIR_CASES[case]
    T1, T2 = (MO.T12, MO.S12) if m == 12 else (MO.T40, MO.S40)
    sq, st = _letters_scores(oracle, pos, "seq", T1, m, 2), _letters_scores(oracle, pos, "struct", T2, m, 2)
    if finite:
        t1, t2 = _seq_struct_thresholds(sq, st, 1000 if joint else 500)
        plain = oracle.stream_hits(sq, st, t1, t2)
        T = _mid(printed_sum(sq[plain], st[plain])) if joint else None
    else:                                              # the joint threshold alone decides: about 3 x 10^-4 of the windows
        t1, t2 = -np.inf, -np.inf
        with np.errstate(invalid="ignore"):
            T = _between_top(sq.astype(F64) + st, 300)
    ctx, o = own.fused, pos.out
    a, b = ctx.motif(T1, None), ctx.motif(T2, None)
    try:
        _zero(pos)
        if joint:
            ctx.hits_pair_sum_dev(a, b, pos.codes.data_ptr(), pos.codes2.data_ptr(), N_POS, t1, t2, T, CAP, o.pos.data_ptr(), o.sq.data_ptr(),
                                  o.st.data_ptr(), o.cnt.data_ptr())
        else:
            ctx.hits_pair_dev(a, b, pos.codes.data_ptr(), pos.codes2.data_ptr(), N_POS, t1, t2, CAP, o.pos.data_ptr(), o.sq.data_ptr(),
                              o.st.data_ptr(), o.cnt.data_ptr())
        ctx.synchronize()
        assert ctx.pair_sum_route() == getattr(_lib, "PAIR_ROUTE_" + route), (case, ctx.pair_sum_route())
    finally:
        a.close()
        b.close()
    hits = _collect(pos)
    _inside(pos, hits, m)
    for i in range(3):
        wsq, wst = _letters_scores(oracle, pos, "seq", T1, m, i), _letters_scores(oracle, pos, "struct", T2, m, i)
        wp = _pair_want(oracle, wsq, wst, m, t1, t2, T)
        gp, gq, gt = _in_slice(pos, i, hits, m)
        assert np.array_equal(gp, wp), "%s, slice at %d: %d hits, the oracle has %d" % (case, pos.lo[i], gp.size, wp.size)
        assert_f32_bits_equal(gq, wsq[wp])
        assert np.array_equal(gt.view(np.uint64), wst[wp].view(np.uint64))
        if joint and finite:
            assert wp.size < _pair_want(oracle, wsq, wst, m, t1, t2, None).size, "the joint threshold drops nothing here"
    _border(pos, hits, m, "two streams, " + case)
    if m == 12:
        assert bool((hits[0] == pos.planted).any()), "the window planted at %d is not among the hits" % pos.planted


def _letter_library_scan(own, box, lib, two_fasta, ts, tt, tj=None):
    ctx, o = own.fused, box.out
    _zero(box)
    first, second = (box.codes.data_ptr(), box.codes2.data_ptr()) if two_fasta else (box.codes2.data_ptr(), None)
    if tj is None:
        ctx.library_hits_letters_dev(lib, first, second, box.n_pos, ts, tt, CAP, o.pos.data_ptr(), o.mo.data_ptr(), o.sq.data_ptr(), o.st.data_ptr(),
                                     o.cnt.data_ptr())
    else:
        ctx.library_hits_letters_sum_dev(lib, first, second, box.n_pos, ts, tt, tj, CAP, o.pos.data_ptr(), o.mo.data_ptr(), o.sq.data_ptr(),
                                         o.st.data_ptr(), o.cnt.data_ptr())
    ctx.synchronize()
    return _collect(box, lib.n)


def _letter_library_case(own, oracle, pos):
    """k_library8: 20 structure-letter motifs over the 8-code stream, two spans of its own"""
    n, what = MO.L8.shape[0], "structure-letter library of 20"
    full = [[_letters_scores(oracle, pos, "struct", MO.L8[k], ("L8", k), i) for k in range(n)] for i in range(3)]
    thr = np.array([_between_top(full[2][k], 30) for k in range(n)])
    lib = own.fused.library(None, struct_letters=MO.L8)
    try:
        hits = _letter_library_scan(own, pos, lib, False, None, thr)
        assert lib.last_launches() == {"n_launches": 2 * lib.info()["passes"], "n_team_launches": 0, "max_teams": 1}
    finally:
        lib.close()
    _inside(pos, hits, 12)
    for i in range(3):
        gp, gm, _, gt = _in_slice(pos, i, hits, 12)
        for k in range(n):
            wp = oracle.stream_hits(None, full[i][k], -np.inf, thr[k])
            wp = wp[wp <= SLICE - 12]
            sel = gm == k
            assert np.array_equal(gp[sel], wp), "%s, motif %d, slice at %d: %d hits, the oracle has %d" % (what, k, pos.lo[i], int(sel.sum()), wp.size)
            assert np.array_equal(gt[sel].view(np.uint64), full[i][k][wp].view(np.uint64))
    _border(pos, hits, 12, what)
    assert bool(((hits[0] == pos.planted) & (hits[1] == 0)).any()), "motif 0's window planted at %d is not among the hits" % pos.planted


def _two_fasta_case(own, oracle, pos, joint):
    """k_library with the second code stream as its structure side: 20 pairs, 8 of them against the oracle"""
    n, what = MO.PT.shape[0], "two-FASTA library of 20, %s" % ("joint" if joint else "plain")
    key = ("pairlib", joint)
    if key not in pos.cache:                           # per-pair thresholds from the tail slice
        ts, tt, tj = np.empty(n), np.empty(n), np.full(n, -np.inf)
        for k in range(n):
            sq, st = _letters_scores(oracle, pos, "seq", MO.PT[k], ("PT", k), 2), _letters_scores(oracle, pos, "struct", MO.PS[k], ("PS", k), 2)
            ts[k], tt[k] = _seq_struct_thresholds(sq, st, 60 if joint else 30)
            if joint:
                plain = oracle.stream_hits(sq, st, ts[k], tt[k])
                tj[k] = _mid(printed_sum(sq[plain], st[plain]))
        pos.cache[key] = (ts, tt, tj)
    ts, tt, tj = pos.cache[key]
    lib = own.fused.library(MO.PT, struct_letters=MO.PS)
    try:
        hits = _letter_library_scan(own, pos, lib, True, ts, tt, tj if joint else None)
    finally:
        lib.close()
    _inside(pos, hits, 12)
    assert int(pos.torch.bincount(hits[1].long(), minlength=n).min()) > 0
    rng = np.random.default_rng(9)
    sel = np.array(sorted({0, n - 1} | set(int(k) for k in rng.permutation(np.arange(1, n - 1))[:6])))
    for i in range(3):
        gp, gm, gq, gt = _in_slice(pos, i, hits, 12)
        for k in sel:
            wsq, wst = _letters_scores(oracle, pos, "seq", MO.PT[k], ("PT", k), i), _letters_scores(oracle, pos, "struct", MO.PS[k], ("PS", k), i)
            wp = _pair_want(oracle, wsq, wst, 12, ts[k], tt[k], tj[k] if joint else None)
            at = gm == k
            assert np.array_equal(gp[at], wp), "%s, pair %d, slice at %d: %d hits, the oracle has %d" % (what, k, pos.lo[i], int(at.sum()), wp.size)
            assert_f32_bits_equal(gq[at], wsq[wp])
            assert np.array_equal(gt[at].view(np.uint64), wst[wp].view(np.uint64))
            if joint:
                assert wp.size < _pair_want(oracle, wsq, wst, 12, ts[k], tt[k], None).size, "the joint threshold drops nothing here"
    keep = pos.torch.isin(hits[1], pos.torch.from_numpy(sel).to(pos.dev).int())
    mine = tuple(x[keep] for x in hits)
    _border(pos, mine, 12, what + ", the 8 pairs checked")
    assert bool(((hits[0] == pos.planted) & (hits[1] == 0)).any()), "pair 0's window planted at %d is not among the hits" % pos.planted


def _wide_letters_case(own, oracle, pos):
    """k_wide_letters at w = 100: all scores (float32, 8.6 GB of output) and hits"""
    from rnascan_amd import _lib
    torch, ctx, o, m = pos.torch, own.fused, pos.out, 100
    _need(torch, 10, "the float32 scores of every position")
    motif = ctx.motif(MO.T100, None)
    out = torch.empty(N_POS, dtype=torch.float32, device=pos.dev)
    try:
        torch.cuda.synchronize()
        ctx.scan_dev(motif, pos.codes.data_ptr(), None, _lib.PROFILE_NONE, N_POS, out.data_ptr(), None)
        ctx.synchronize()
        full = [_letters_scores(oracle, pos, "seq", MO.T100, 100, i) for i in range(3)]
        for i in range(3):
            assert_f32_bits_equal(out[pos.lo[i]:pos.lo[i] + SLICE - m + 1].cpu().numpy(), full[i][:SLICE - m + 1])
        del out
        torch.cuda.empty_cache()
        thr = _kth_below(full[2], 500)
        _zero(pos)
        ctx.hits_dev(motif, pos.codes.data_ptr(), None, _lib.PROFILE_NONE, N_POS, thr, -np.inf, CAP, o.pos.data_ptr(), o.sq.data_ptr(), None,
                     o.cnt.data_ptr())
        ctx.synchronize()
    finally:
        motif.close()
    hits = _collect(pos)
    _inside(pos, hits, m)
    for i in range(3):
        wp = oracle.stream_hits(full[i], None, thr, -np.inf)
        wp = wp[wp <= SLICE - m]
        gp, gq, _ = _in_slice(pos, i, hits, m)
        assert np.array_equal(gp, wp), "slice at %d: %d hits, the oracle has %d" % (pos.lo[i], gp.size, wp.size)
        assert_f32_bits_equal(gq, full[i][wp])
    _border(pos, hits, m, "wide letters w100")


# ---- the cases, one class per stream: its fixtures are class-scoped, so one stream is resident at a time ------------------------
TEAMS = {"n_launches": 1, "n_team_launches": 1, "max_teams": 2}
ONE_BY_ONE = {"n_launches": 2, "n_team_launches": 0, "max_teams": 1}


class TestBeyondTwoToThe31ProfileElements(object):
    """the stream `elem`: B1 and B2"""

    @pytest.mark.parametrize("case", list(SINGLE_CASES))
    def test_single_motif_hits(self, own, oracle, elem, case):
        _single_case(own, oracle, elem, case)

    @pytest.mark.parametrize("kind", ["plain", "plain, float64 rows", "joint"])
    def test_library_teams(self, lib_elem, kind):
        """k_library phase B (lib_struct_score: 64-bit row addresses from pos_base + rel), plain and SUM, two teams in one launch"""
        _library_case(lib_elem, kind, TEAMS, ONE_BY_ONE)

    @pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
    def test_structure_only_library(self, own, oracle, elem, dtype):
        _struct_library_case(own, oracle, elem, dtype)

    def test_library_site_sums(self, lib_elem):
        _site_sums_case(lib_elem)


class TestBeyondTwoToThe31Positions(object):
    """the letter streams `pos`: B3"""

    @pytest.mark.parametrize("case", list(PAIR_CASES))
    def test_two_stream_hits(self, own, oracle, pos, case):
        _pair_case(own, oracle, pos, case)

    def test_structure_letter_library(self, own, oracle, pos):
        _letter_library_case(own, oracle, pos)

    @pytest.mark.parametrize("joint", [False, True], ids=["plain", "joint"])
    def test_two_fasta_library(self, own, oracle, pos, joint):
        _two_fasta_case(own, oracle, pos, joint)

    def test_wide_letters(self, own, oracle, pos):
        _wide_letters_case(own, oracle, pos)


class TestBeyondTwoToThe31PositionsWithAProfile(object):
    """the stream `pos_prof`: B3 with a profile"""

    @pytest.mark.parametrize("case", ["fused w12 (k_profile_fixed)", "joint w12 (k_profile_fixed_sum)"])
    def test_single_motif_hits(self, own, oracle, pos_prof, case):
        _single_case(own, oracle, pos_prof, case)

    @pytest.mark.parametrize("kind", ["plain", "joint"])
    def test_library_short_last_span(self, lib_prof, kind):
        """lib_run's second span (pos_base = 2^31) has 92 work segments, fewer than the CUs: one team launch for the first span,
        then the two passes of the last span one by one"""
        assert -(-(N_POS - (1 << 31)) // 16384) == 92 < lib_prof.own.n_cu
        _library_case(lib_prof, kind, {"n_launches": 3, "n_team_launches": 1, "max_teams": 2}, {"n_launches": 4, "n_team_launches": 0, "max_teams": 1})

    def test_structure_only_library(self, own, oracle, pos_prof):
        _struct_library_case(own, oracle, pos_prof, F32)

