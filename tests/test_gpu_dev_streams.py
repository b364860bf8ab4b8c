"""The device-resident entry points (`_dev`, include/pfmscan.h) as an integrator calls them: on the CALLER's stream, and with
hit buffers smaller than the number of hits.

A. Ordering on a caller's stream.  Every entry point that takes `void *stream` runs behind a long delay on a torch side
stream S: the buffers it reads hold neutral contents (separator codes, zero rows, a non-zero hit counter) until S itself
copies the real inputs in and zeroes the counter -- after the delay --, the entry point is called with stream = S with no
synchronisation anywhere, and S clones the outputs and then overwrites the inputs with garbage.  Whatever step of the entry
point (a memset, a table upload, a count read-back, a helper kernel) ran anywhere but on S has read the neutral contents
or a stale counter, and the clones differ from the reference.  The entry points the header calls asynchronous must also
RETURN while the delay still runs (the event recorded behind the copies has not completed directly after the call); that
proves the contract, and that the delay was long enough for the test to mean anything.

Before the pattern, each case makes the same call once on S, synchronised, on ANOTHER input set of the same shape (`warm`:
the stream read backwards, other structures of the same lengths, other letters) with the same thresholds: that run loads
the kernels, sizes the ctx's scratch (allocating synchronises the device) and is timed with events: the delay lasts at least
20 ms and at least 20 x that time (asserted; the measured figures are in every assertion message).  It leaves the ctx's and
the library's scratch -- candidates and their counts, sharded hits, prefix sums, partial sums -- holding ANOTHER answer
(asserted: its outputs fail the case's check), so an internal step that ran off S and met the scratch of the call before
gives a wrong result as well.  The entry points that read a verdict back are then called once more on an input they reject,
so the stale verdict is a rejection; those that read candidate counts back only to choose their route (hits_core, pair_core)
once more on the neutral inputs, so the stale counts say "no candidate" and the route they choose stores no hit.  For a
library the warm run also leaves the thresholds set, which is the condition under which pfmscan_library_hits_dev /
_letters_dev are asynchronous; the follow-up calls then change them.

The limit of the pattern: a KERNEL launched on another stream is caught only when that stream really runs beside S (two
streams that share a hardware queue run in order); read-backs and copies issued from the host are caught in every case.

B. Capacity on the single-motif hit forms: with room for a third of the hits the count still reports all of them, the
stored ones are distinct hits with their own scores, and nothing is written behind `capacity`."""
import math

import numpy as np
import pytest

from conftest import assert_f32_bits_equal
from precision_rules import assert_struct_tight
import test_gpu_average_dev as avg                        # its random set, table builder and numpy reference
# generators and threshold pickers of the suites of the same kernels; the underscore names are those modules' own helpers,
# used here as they stand so that both files draw the same kind of stream: a rename there has to be followed here
from test_gpu_letters8 import _between, _stream as letter_stream, _table as letter_table
from test_gpu_library import _clear_of, check as check_library_hits, make_library, oracle_library_hits, quantile_thresholds
from test_gpu_library8 import _pair_stream
from test_gpu_parity import rand_stream, rand_struct_pssm, rand_table

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL_COUNT = 12345


# ---- the delay and the pattern -----------------------------------------------------------------------------------------
class Delay(object):
    """ordinary torch work of a known length: in-place passes over a 1 GiB tensor, one pass timed with events"""

    def __init__(self):
        import torch
        self.x = torch.zeros(1 << 28, dtype=torch.float32, device=DEV)
        for _ in range(3):
            self.x.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(8):
            self.x.add_(1.0)
        e1.record()
        e1.synchronize()
        self.ms_per_pass = e0.elapsed_time(e1) / 8

    def enqueue(self, ms):
        """at least `ms` of work on the current stream (twice the passes the measurement asks for)"""
        for _ in range(int(math.ceil(2.0 * ms / self.ms_per_pass))):
            self.x.add_(1.0)


@pytest.fixture(scope="module")
def delay():
    d = Delay()
    yield d
    del d.x


def _to_dev(arrays):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in arrays.items()}


class Case(object):
    """one entry point at one shape.
    real / neutral / garbage: name -> numpy array (the inputs, what they hold before S copies them in, what S leaves behind)
    warm: another input set of the same shape, for the timed run that leaves the scratch holding another answer
    rejected: None, or an input set of the same shape that the entry point rejects with ValueError
    count_read_back: the entry point reads candidate counts back and chooses its route by them: a run on the neutral inputs,
      which have no candidate, follows the warm run, so counts read from the scratch of the call before say "no candidate"
    make_outs() -> (name -> device tensor holding sentinels, names S zeroes before the call)
    call(buf, outs, stream, alt) runs the entry point on the device tensors; check(out, msg, alt) compares numpy copies of
    the outputs with the reference (alt: a library's second set of thresholds)"""
    asynchronous = False
    library = False
    rejected = None
    count_read_back = False

    def close(self):
        pass


def _timed_plain_run(case, S):
    """the call on S with the `warm` inputs in place, synchronised: loads the kernels, sizes the scratch and leaves another
    answer in it -> (its time in ms, its outputs as numpy)"""
    import torch
    buf = _to_dev(case.warm)
    outs, zero = case.make_outs()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        e0.record(S)
        for k in zero:
            outs[k].zero_()
    case.call(buf, outs, S.cuda_stream, False)
    with torch.cuda.stream(S):
        e1.record(S)
    S.synchronize()
    return e0.elapsed_time(e1), {k: v.cpu().numpy() for k, v in outs.items()}


def _one_more_plain_run(case, S, arrays, rejected):
    """one synchronised call on S on `arrays`: an input the entry point rejects (the verdict in the ctx's scratch is then a
    rejection), or one without a candidate (the candidate counts in the ctx's scratch are then zero)"""
    import torch
    buf = _to_dev(arrays)
    outs, zero = case.make_outs()
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        for k in zero:
            outs[k].zero_()
    if rejected:
        with pytest.raises(ValueError):
            case.call(buf, outs, S.cuda_stream, False)
    else:
        case.call(buf, outs, S.cuda_stream, False)
    S.synchronize()


def _backwards(arrays):
    """the same streams read from their end: the same shape and the same letters and rows, other windows"""
    return {k: np.ascontiguousarray(v[::-1]) for k, v in arrays.items()}


def _behind_delay(case, delay, S, need_ms):
    """-> ([outputs of every call as numpy], [did the call return before its inputs were ready], measured delay in ms)"""
    import torch
    src, junk, buf = _to_dev(case.real), _to_dev(case.garbage), _to_dev(case.neutral)
    calls = [False, False, True] if case.library else [False]          # a library: the same thresholds again, then others
    all_outs = [case.make_outs() for _ in calls]
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    clones, pending = [], []
    for i, alt in enumerate(calls):
        outs, zero = all_outs[i]
        if i < 2:                                        # (the call with other thresholds follows its predecessor directly)
            with torch.cuda.stream(S):
                if i == 0:
                    t0.record(S)
                delay.enqueue(need_ms)
                if i == 0:
                    t1.record(S)
                for k in buf:
                    buf[k].copy_(src[k])
                for k in zero:
                    outs[k].zero_()
                ready = torch.cuda.Event()
                ready.record(S)
        else:
            with torch.cuda.stream(S):
                for k in zero:
                    outs[k].zero_()
        case.call(buf, outs, S.cuda_stream, alt)         # no synchronisation anywhere
        pending.append(not ready.query() if i < 2 else None)      # (the third call has no delay in front of it)
        with torch.cuda.stream(S):
            clones.append({k: v.clone() for k, v in outs.items()})
            if i + 1 == len(calls) or i == 0:
                for k in buf:
                    buf[k].copy_(junk[k])
    S.synchronize()
    return [{k: v.cpu().numpy() for k, v in c.items()} for c in clones], pending, t0.elapsed_time(t1)


# ---- shared inputs -----------------------------------------------------------------------------------------------------
def _garbage_like(rng, a):
    if a.dtype == np.uint8:
        return rng.integers(0, 8, size=a.shape).astype(np.uint8)
    if a.dtype.kind == "f":
        return rng.random(a.shape).astype(a.dtype)
    return np.zeros_like(a)                              # index tables: harmless values


def _hit_outs(cap, with_motif=False, seq=True, st=True, zero_count=True):
    import torch
    outs = {"pos": torch.full((cap,), -1, dtype=torch.int64, device=DEV)}
    if with_motif:
        outs["motif"] = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
    if seq:
        outs["seq"] = torch.full((cap,), -3.0, dtype=torch.float32, device=DEV)
    if st:
        outs["st"] = torch.full((cap,), -3.0, dtype=torch.float64, device=DEV)
    outs["count"] = torch.full((1,), SENTINEL_COUNT, dtype=torch.int64, device=DEV)
    return outs, (["count"] if zero_count else [])


def _ptr(outs, name):
    return outs[name].data_ptr() if name in outs else None


def _check_hits(out, want_pos, want_seq=None, struct=None, exact=None, msg=""):
    """the device's unordered hits, sorted, against the oracle's: count, positions, float32 bits, structure scores"""
    k = int(out["count"][0])
    assert k == len(want_pos) and k > 20, "%d hits, the oracle has %d; %s" % (k, len(want_pos), msg)
    order = np.argsort(out["pos"][:k], kind="stable")
    assert np.array_equal(out["pos"][:k][order], want_pos), msg
    if want_seq is not None:
        assert_f32_bits_equal(out["seq"][:k][order], want_seq[want_pos])
    if struct is not None:
        assert_struct_tight(out["st"][:k][order], struct[0], struct[1], positions=want_pos)
    if exact is not None:
        assert np.array_equal(out["st"][:k][order], exact[want_pos]), msg


class _SeqStruct(Case):
    """a packed stream of ~30 records of 0..700 positions, a motif with both parts, m = 12"""

    def __init__(self, ctx, oracle, dtype=np.float32, seed=5):
        from rnascan_amd import _lib, pack
        self.ctx = ctx
        rng = np.random.default_rng(seed)
        self.s = s = rand_stream(rng, 30, 0, 700, dtype=dtype)
        self.T, self.P = rand_table(rng, 12), rand_struct_pssm(rng, 12)
        self.motif = ctx.motif(self.T, self.P)
        self.dt = _lib.PROFILE_F32 if dtype == np.float32 else _lib.PROFILE_F64
        self.want_seq, self.want_st = oracle.stream_seq(s.codes, self.T), oracle.stream_struct(s.profile, self.P)
        self.real = {"codes": s.codes, "profile": s.profile}
        self.neutral = {"codes": np.full_like(s.codes, pack.SEP), "profile": np.zeros_like(s.profile)}
        self.garbage = {k: _garbage_like(rng, v) for k, v in self.real.items()}
        self.warm = _backwards(self.real)

    def close(self):
        self.motif.close()


class ScanDev(_SeqStruct):
    asynchronous = True

    def make_outs(self):
        import torch
        n = self.s.n_pos
        return {"seq": torch.full((n,), -3.0, dtype=torch.float32, device=DEV),
                "st": torch.full((n,), -3.0, dtype=torch.float64, device=DEV)}, []

    def call(self, buf, outs, stream, alt):
        self.ctx.scan_dev(self.motif, buf["codes"].data_ptr(), buf["profile"].data_ptr(), self.dt, self.s.n_pos,
                          outs["seq"].data_ptr(), outs["st"].data_ptr(), stream)

    def check(self, out, msg, alt):
        assert_f32_bits_equal(out["seq"], self.want_seq)
        assert_struct_tight(out["st"], self.s.profile, self.P)


class HitsDev(_SeqStruct):
    asynchronous = True
    adaptive = False

    def __init__(self, ctx, oracle):
        _SeqStruct.__init__(self, ctx, oracle)
        fs, ft = self.want_seq[np.isfinite(self.want_seq)], self.want_st[np.isfinite(self.want_st)]
        # 0.985: selective, the two-phase route of pfmscan_hits_adaptive_dev at this size
        self.thr_seq = float(np.quantile(fs, 0.985 if self.adaptive else 0.8))
        self.thr_st = float(np.quantile(ft, 0.4))
        self.want_pos = oracle.stream_hits(self.want_seq, self.want_st, self.thr_seq, self.thr_st)

    def make_outs(self):
        return _hit_outs(self.s.n_pos)

    def call(self, buf, outs, stream, alt):
        f = self.ctx.hits_adaptive_dev if self.adaptive else self.ctx.hits_dev
        f(self.motif, buf["codes"].data_ptr(), buf["profile"].data_ptr(), self.dt, self.s.n_pos, self.thr_seq, self.thr_st,
          self.s.n_pos, _ptr(outs, "pos"), _ptr(outs, "seq"), _ptr(outs, "st"), _ptr(outs, "count"), stream)

    def check(self, out, msg, alt):
        _check_hits(out, self.want_pos, self.want_seq, (self.s.profile, self.P), msg=msg)


class HitsAdaptiveDev(HitsDev):
    asynchronous = False                                  # the header: synchronises `stream`
    adaptive = True
    count_read_back = True                                # hits_core


class _Letters(Case):
    """a 7-letter code stream (case bits, foreign letters), a letters-only motif, m = 8, fp64 scores"""

    def __init__(self, ctx, oracle):
        from rnascan_amd import pack
        self.ctx = ctx
        rng = np.random.default_rng(8)
        self.s = s = letter_stream(rng, [int(x) for x in rng.integers(0, 701, size=30)])
        self.T = letter_table(rng, 8)
        self.motif = ctx.motif(self.T, None)
        self.full = oracle.stream_letters_f64(s.codes, self.T)
        self.thr = _between(self.full, 0.97)
        self.want_pos = oracle.stream_hits(None, self.full, -np.inf, self.thr)
        self.real = {"codes": s.codes}
        self.neutral = {"codes": np.full_like(s.codes, pack.SEP)}
        self.garbage = {"codes": _garbage_like(rng, s.codes)}
        self.warm = _backwards(self.real)

    def close(self):
        self.motif.close()


class ScanLettersF64Dev(_Letters):
    asynchronous = True

    def make_outs(self):
        import torch
        return {"score": torch.full((self.s.n_pos,), -3.0, dtype=torch.float64, device=DEV)}, []

    def call(self, buf, outs, stream, alt):
        self.ctx.scan_letters_f64_dev(self.motif, buf["codes"].data_ptr(), self.s.n_pos, outs["score"].data_ptr(), stream)

    def check(self, out, msg, alt):
        got, want = out["score"], self.full
        assert np.array_equal(np.isnan(got), np.isnan(want)), msg
        assert np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)]), msg     # the same sequential fp64 sum


class HitsLettersF64Dev(_Letters):
    asynchronous = True

    def make_outs(self):
        return _hit_outs(self.s.n_pos, seq=False)

    def call(self, buf, outs, stream, alt):
        self.ctx.hits_letters_f64_dev(self.motif, buf["codes"].data_ptr(), self.s.n_pos, self.thr, self.s.n_pos,
                                      _ptr(outs, "pos"), _ptr(outs, "st"), _ptr(outs, "count"), stream)

    def check(self, out, msg, alt):
        _check_hits(out, self.want_pos, exact=self.full, msg=msg)


class HitsPairDev(Case):
    """sequence letters AND structure letters of the same records, both PFMs 12 wide"""
    count_read_back = True                                # pair_core, under PFMSCAN_PAIR_TWO_PHASE=1

    def __init__(self, ctx, oracle, q_seq=0.95):
        from rnascan_amd import pack
        self.ctx = ctx
        rng = np.random.default_rng(13)
        self.a, self.b = _pair_stream(rng, [int(x) for x in rng.integers(0, 701, size=30)])
        self.T, self.ST = rand_table(rng, 12), letter_table(rng, 12)
        self.mo_seq, self.mo_st = ctx.motif(self.T, None), ctx.motif(self.ST, None)
        self.fs, self.ft = oracle.stream_seq(self.a.codes, self.T), oracle.stream_letters_f64(self.b.codes, self.ST)
        self.thr_seq = float(np.quantile(self.fs[np.isfinite(self.fs)], q_seq)) + 1e-4
        self.thr_st = _between(self.ft, 0.5)
        self.want_pos = oracle.stream_hits(self.fs, self.ft, self.thr_seq, self.thr_st)
        self.n = self.a.codes.size
        self.real = {"codes": self.a.codes, "codes2": self.b.codes}
        self.neutral = {k: np.full_like(v, pack.SEP) for k, v in self.real.items()}
        self.garbage = {k: _garbage_like(rng, v) for k, v in self.real.items()}
        self.warm = _backwards(self.real)

    def make_outs(self):
        return _hit_outs(self.n)

    def call(self, buf, outs, stream, alt):
        self.ctx.hits_pair_dev(self.mo_seq, self.mo_st, buf["codes"].data_ptr(), buf["codes2"].data_ptr(), self.n, self.thr_seq,
                               self.thr_st, self.n, _ptr(outs, "pos"), _ptr(outs, "seq"), _ptr(outs, "st"), _ptr(outs, "count"),
                               stream)

    def check(self, out, msg, alt):
        _check_hits(out, self.want_pos, self.fs, exact=self.ft, msg=msg)

    def close(self):
        self.mo_seq.close()
        self.mo_st.close()


class _Library(Case):
    asynchronous = True                                   # while the thresholds repeat (include/pfmscan.h)
    library = True

    def make_outs(self):
        # the library forms do not need a zeroed count: k_lib_prefix writes the total.  The sentinel stays until it does, and
        # the total it would write from the scratch of the warm run is another one
        return _hit_outs(self.cap, with_motif=True, zero_count=False)

    def _sorted(self, out, want_k, msg):
        k = int(out["count"][0])
        assert k == want_k and k > 20, "%d hits, the oracle has %d; %s" % (k, want_k, msg)
        order = np.lexsort((out["motif"][:k], out["pos"][:k]))
        return out["pos"][:k][order], out["motif"][:k][order], out["seq"][:k][order], out["st"][:k][order]

    def close(self):
        self.lib.close()


class LibraryCombined(_Library):
    """k_library: 8 motifs with both parts over codes + profile"""

    def __init__(self, ctx, oracle):
        from rnascan_amd import _lib, pack
        self.ctx = ctx
        rng = np.random.default_rng(21)
        self.s = s = rand_stream(rng, 30, 0, 700)
        self.LT, self.LP = make_library(rng, 8, 12)
        self.lib = ctx.library(self.LT, self.LP)
        self.dt = _lib.PROFILE_F32
        self.thr = [quantile_thresholds(oracle, s, self.LT, self.LP, 0.95, 0.4), quantile_thresholds(oracle, s, self.LT, self.LP, 0.9, 0.6)]
        self.want = [oracle_library_hits(oracle, s, self.LT, self.LP, ts, tt) for ts, tt in self.thr]
        self.cap = max(len(w[0]) for w in self.want) + 64
        self.real = {"codes": s.codes, "profile": s.profile}
        self.neutral = {"codes": np.full_like(s.codes, pack.SEP), "profile": np.zeros_like(s.profile)}
        self.garbage = {k: _garbage_like(rng, v) for k, v in self.real.items()}
        self.warm = _backwards(self.real)

    def call(self, buf, outs, stream, alt):
        ts, tt = self.thr[int(alt)]
        self.ctx.library_hits_dev(self.lib, buf["codes"].data_ptr(), buf["profile"].data_ptr(), self.dt, self.s.n_pos, ts, tt, self.cap,
                                  _ptr(outs, "pos"), _ptr(outs, "motif"), _ptr(outs, "seq"), _ptr(outs, "st"), _ptr(outs, "count"), stream)

    def check(self, out, msg, alt):
        want = self.want[int(alt)]
        pos, mot, sq, st = self._sorted(out, len(want[0]), msg)
        check_library_hits((pos, mot, sq, st), want, True)
        for k in range(self.LT.shape[0]):
            sel = mot == k
            assert_struct_tight(st[sel], self.s.profile, self.LP[k], positions=pos[sel])


class LibraryStructOnly(_Library):
    """k_profile_lib: 6 structure PSSMs over the profile alone (no codes: no separators)"""

    def __init__(self, ctx, oracle):
        from rnascan_amd import _lib
        self.ctx = ctx
        rng = np.random.default_rng(22)
        self.s = s = rand_stream(rng, 30, 0, 700)
        self.LP = np.stack([rand_struct_pssm(rng, 12) for _ in range(6)])
        self.lib = ctx.library(None, self.LP)
        self.dt = _lib.PROFILE_F32
        self.st = [oracle.stream_struct(s.profile, P) for P in self.LP]
        self.thr = [np.array([_clear_of(v[np.isfinite(v)], float(np.quantile(v[np.isfinite(v)], q))) for v in self.st]) for q in (0.97, 0.9)]
        self.want = [[oracle.stream_hits(None, v, -np.inf, float(t)) for v, t in zip(self.st, thr)] for thr in self.thr]
        self.cap = max(sum(len(p) for p in w) for w in self.want) + 64
        self.real = {"profile": s.profile}
        self.neutral = {"profile": np.zeros_like(s.profile)}
        self.garbage = {"profile": _garbage_like(rng, s.profile)}
        self.warm = _backwards(self.real)

    def call(self, buf, outs, stream, alt):
        self.ctx.library_hits_dev(self.lib, None, buf["profile"].data_ptr(), self.dt, self.s.n_pos, None, self.thr[int(alt)], self.cap,
                                  _ptr(outs, "pos"), _ptr(outs, "motif"), _ptr(outs, "seq"), _ptr(outs, "st"), _ptr(outs, "count"), stream)

    def check(self, out, msg, alt):
        want = self.want[int(alt)]
        pos, mot, sq, st = self._sorted(out, sum(len(p) for p in want), msg)
        assert np.isnan(sq).all(), msg                    # no sequence side
        for k, P in enumerate(self.LP):
            sel = mot == k
            assert np.array_equal(pos[sel], want[k]), (k, msg)
            assert_struct_tight(st[sel], self.s.profile, P, positions=want[k])


class LibraryLetters(_Library):
    """k_library8 (structure-letter library over one 8-code stream, m = 8), or -- `pair` -- a two-FASTA library (m = 12)"""

    def __init__(self, ctx, oracle, pair=False):
        from rnascan_amd import pack
        self.ctx, self.pair = ctx, pair
        rng = np.random.default_rng(23 + int(pair))
        lengths = [int(x) for x in rng.integers(0, 701, size=30)]
        m, n = (12, 6) if pair else (8, 10)
        if pair:
            self.a, self.b = _pair_stream(rng, lengths)
            self.LT = np.stack([rand_table(rng, m) for _ in range(n)])
        else:
            self.a, self.b, self.LT = None, letter_stream(rng, lengths), None
        self.ST = np.stack([letter_table(rng, m) for _ in range(n)])
        self.lib = ctx.library(self.LT, struct_letters=self.ST)
        self.ft = [oracle.stream_letters_f64(self.b.codes, T) for T in self.ST]
        self.fs = [oracle.stream_seq(self.a.codes, T) for T in self.LT] if pair else [None] * n
        self.thr, self.want = [], []
        for q_seq, q_st in ((0.9, 0.5), (0.8, 0.7)) if pair else ((None, 0.97), (None, 0.9)):
            tt = np.array([_between(f, q_st) for f in self.ft])
            ts = np.array([float(np.quantile(f[np.isfinite(f)], q_seq)) + 1e-4 for f in self.fs]) if pair else None
            self.thr.append((ts, tt))
            self.want.append([oracle.stream_hits(self.fs[k], self.ft[k], ts[k] if pair else -np.inf, float(tt[k])) for k in range(n)])
        self.cap = max(sum(len(p) for p in w) for w in self.want) + 64
        self.n_pos = self.b.codes.size
        self.real = {"codes": self.a.codes, "codes2": self.b.codes} if pair else {"codes": self.b.codes}
        self.neutral = {k: np.full_like(v, pack.SEP) for k, v in self.real.items()}
        self.garbage = {k: _garbage_like(rng, v) for k, v in self.real.items()}
        self.warm = _backwards(self.real)

    def call(self, buf, outs, stream, alt):
        ts, tt = self.thr[int(alt)]
        self.ctx.library_hits_letters_dev(self.lib, buf["codes"].data_ptr(), buf["codes2"].data_ptr() if self.pair else None, self.n_pos,
                                          ts, tt, self.cap, _ptr(outs, "pos"), _ptr(outs, "motif"), _ptr(outs, "seq"), _ptr(outs, "st"),
                                          _ptr(outs, "count"), stream)

    def check(self, out, msg, alt):
        want = self.want[int(alt)]
        pos, mot, sq, st = self._sorted(out, sum(len(p) for p in want), msg)
        for k in range(self.ST.shape[0]):
            sel = mot == k
            assert np.array_equal(pos[sel], want[k]), (k, msg)
            assert np.array_equal(st[sel], self.ft[k][want[k]]), (k, msg)
            if self.pair:
                assert_f32_bits_equal(sq[sel], self.fs[k][want[k]])


class DotbracketAnnotateDev(Case):
    LETTERS = "EHTBLRM"

    def __init__(self, ctx, oracle):
        from dotbracket_rules import annotate, count_letters, random_structure
        from rnascan_amd import dotbracket, pack
        self.ctx = ctx
        rng = np.random.default_rng(31)
        structs = [random_structure(rng, int(L)) for L in rng.integers(1, 701, size=30)]
        self.s = s = pack.pack([dotbracket.LUT[np.frombuffer(t.encode("latin-1"), dtype=np.uint8)] for t in structs])
        lut = np.full(256, pack.SEP, dtype=np.uint8)
        for i, ch in enumerate(self.LETTERS):
            lut[ord(ch)] = i
        self.want = np.full(s.n_pos, pack.SEP, dtype=np.uint8)
        for o, t in zip(s.offsets.tolist(), structs):
            self.want[o:o + len(t)] = lut[np.frombuffer(annotate(t).encode(), dtype=np.uint8)]
        self.want_counts = np.asarray(count_letters("".join(annotate(t) for t in structs)))
        self.real = {"codes": s.codes}
        self.neutral = {"codes": np.full_like(s.codes, pack.SEP)}
        self.garbage = {"codes": rng.choice(np.array([0, 1, 2, 3, 7], dtype=np.uint8), size=s.n_pos)}
        # other structures of the same lengths; and the records with every bracket and dot an opening bracket: unbalanced
        other = pack.pack([dotbracket.LUT[np.frombuffer(random_structure(rng, len(t)).encode("latin-1"), dtype=np.uint8)] for t in structs])
        assert np.array_equal(other.codes == pack.SEP, s.codes == pack.SEP)
        self.warm = {"codes": other.codes}
        self.rejected = {"codes": np.where(s.codes == pack.SEP, s.codes, np.uint8(dotbracket.OPEN)).astype(np.uint8)}

    def make_outs(self):
        import torch
        return {"letters": torch.full((self.s.n_pos,), 99, dtype=torch.uint8, device=DEV),
                "counts": torch.full((7,), -1, dtype=torch.int64, device=DEV)}, []

    def call(self, buf, outs, stream, alt):
        self.ctx.dotbracket_annotate_dev(buf["codes"], outs["letters"], self.s.n_pos, d_counts=outs["counts"], stream=stream)

    def check(self, out, msg, alt):
        assert np.array_equal(out["letters"], self.want), msg
        assert np.array_equal(out["counts"], self.want_counts), msg


class AverageDev(Case):
    """tests/test_gpu_average_dev.py's random set and numpy reference; the letters are neutral (codes that count for nothing:
    every row uncovered, a rejection) until S copies them in"""

    def __init__(self, ctx, oracle):
        self.ctx = ctx
        rng = np.random.default_rng(41)
        recs = avg.random_set(rng)
        t, self.n_rows, self.longest = avg.build_tables(recs)
        T = avg.value_table()
        self.want = avg.want_rows(recs, T, np.float64)
        self.real = dict(t, table=T)
        self.neutral = dict(self.real, letters=np.full_like(t["letters"], 7))
        self.garbage = {k: _garbage_like(rng, v) for k, v in self.real.items()}
        # every counted letter turned into its neighbour: the same coverage, other rows; the neutral letters are a rejection
        self.warm = dict(self.real, letters=np.where(t["letters"] < 7, (t["letters"] + 1) % 7, t["letters"]).astype(np.uint8))
        self.rejected = self.neutral

    def make_outs(self):
        import torch
        return {"rows": torch.full((self.n_rows, 7), -7.0, dtype=torch.float64, device=DEV)}, []

    def call(self, buf, outs, stream, alt):
        avg.call_average(self.ctx, buf, self.n_rows, self.longest, outs["rows"], np.float64, stream=stream)

    def check(self, out, msg, alt):
        assert avg.same_bits(out["rows"], self.want), msg


class ProfileColsumsDev(Case):
    def __init__(self, ctx, oracle):
        import background_rules as rules
        self.ctx = ctx
        rng = np.random.default_rng(51)
        self.s = s = rand_stream(rng, 30, 0, 700)
        self.want = rules.colsums(s.profile, s.offsets, s.lengths)           # the restatement of the order of additions: bit for bit
        self.real = {"profile": s.profile, "offsets": np.ascontiguousarray(s.offsets, dtype=np.int64),
                     "lengths": np.ascontiguousarray(s.lengths, dtype=np.int64)}
        self.neutral = dict(self.real, profile=np.zeros_like(s.profile))
        self.garbage = {k: _garbage_like(rng, v) for k, v in self.real.items()}
        self.warm = dict(self.real, profile=np.ascontiguousarray(s.profile[::-1]))      # other rows under the same records
        bad = s.profile.copy()
        bad[int(s.offsets[np.flatnonzero(s.lengths > 0)[0]]), 0] = -1.0                 # a negative cell inside a record
        self.rejected = dict(self.real, profile=bad)

    def make_outs(self):
        import torch
        return {"sums": torch.full((len(self.s.offsets), 7), -1.0, dtype=torch.float64, device=DEV)}, []

    def call(self, buf, outs, stream, alt):
        self.ctx.profile_colsums_dev(buf["profile"], np.float32, self.s.n_pos, buf["offsets"], buf["lengths"], len(self.s.offsets),
                                     outs["sums"], stream=stream)

    def check(self, out, msg, alt):
        assert self.want.any() and np.array_equal(out["sums"].view(np.int64), self.want.view(np.int64)), msg
        # ... and a plain float64 numpy sum of every record agrees to rounding
        plain = np.array([self.s.profile[o:o + n].astype(np.float64).sum(axis=0) for o, n in zip(self.s.offsets, self.s.lengths)])
        assert np.allclose(out["sums"], plain, rtol=1e-12, atol=1e-12), msg


CASES = {
    "scan_dev": lambda c, o: ScanDev(c, o),
    "scan_dev_float64_rows": lambda c, o: ScanDev(c, o, dtype=np.float64, seed=6),
    "scan_letters_f64_dev": ScanLettersF64Dev,
    "hits_dev": HitsDev,
    "hits_adaptive_dev": HitsAdaptiveDev,
    "hits_letters_f64_dev": HitsLettersF64Dev,
    "hits_pair_dev": HitsPairDev,
    "hits_pair_dev_two_phase": HitsPairDev,               # PFMSCAN_PAIR_TWO_PHASE=1 in a fresh context: pair_core's candidate route
    "library_hits_dev": LibraryCombined,
    "library_hits_dev_structure_only": LibraryStructOnly,
    "library_hits_letters_dev": LibraryLetters,
    "library_hits_letters_dev_two_fasta": lambda c, o: LibraryLetters(c, o, pair=True),
    "dotbracket_annotate_dev": DotbracketAnnotateDev,
    "average_dev": AverageDev,
    "profile_colsums_dev": ProfileColsumsDev,
}


@pytest.mark.parametrize("name", list(CASES))
def test_entry_point_works_in_the_order_of_the_callers_stream(name, ctx, oracle, delay, monkeypatch):
    import torch
    from rnascan_amd import _lib
    own = None
    if name == "hits_pair_dev_two_phase":
        monkeypatch.setenv("PFMSCAN_PAIR_TWO_PHASE", "1")
        own = ctx = _lib.Context(0)
    case = CASES[name](ctx, oracle)
    S = torch.cuda.Stream()
    try:
        own_ms, warm_outs = _timed_plain_run(case, S)
        with pytest.raises(AssertionError):              # what that run left in the scratch is ANOTHER answer
            case.check(warm_outs, "the warm run", False)
        if case.count_read_back:
            _one_more_plain_run(case, S, case.neutral, False)
        if case.rejected is not None:
            _one_more_plain_run(case, S, case.rejected, True)
        need_ms = max(20.0, 20.0 * own_ms)
        outs, pending, delay_ms = _behind_delay(case, delay, S, need_ms)
        msg = "delay %.1f ms (%.1f ms asked for: 20 x the call's own %.3f ms, at least 20 ms; one pass %.3f ms)" % (
            delay_ms, need_ms, own_ms, delay.ms_per_pass)
        assert delay_ms >= need_ms, "the delay was too short for the test to mean anything: " + msg
        if case.asynchronous:
            assert pending[0], "the call returned only after the work queued in front of it had run: not asynchronous; " + msg
        case.check(outs[0], msg, False)
        if case.library:
            # the same thresholds again, still without a synchronisation: asynchronous, the same hits
            assert pending[1], "the repeated call with the same thresholds was not asynchronous; " + msg
            case.check(outs[1], "repeated call; " + msg, False)
            assert int(outs[1]["count"][0]) == int(outs[0]["count"][0]), msg
            # other thresholds directly behind it: that call got ITS thresholds (pfmscan_library_hits_*_dev synchronises the
            # stream before it rewrites the library's threshold table), and so did this one
            case.check(outs[2], "call with other thresholds; " + msg, True)
    finally:
        torch.cuda.synchronize()
        case.close()
        if own is not None:
            own.close()


# ---- B. capacity below the number of hits ------------------------------------------------------------------------------
class _Capacity(object):
    """hits of one single-motif `_dev` form: run(n_pos, capacity, pos, seq, st, count) with device tensors or None"""

    def __init__(self, kind, ctx, oracle):
        from rnascan_amd import _lib
        import torch
        rng = np.random.default_rng(61)
        self.kind, self.ctx = kind, ctx
        self.seq_scores = self.struct = self.exact = None
        self.motifs = []
        if kind in ("hits_dev_letters", "hits_dev_struct", "hits_dev_both", "hits_adaptive_dev"):
            s = rand_stream(rng, 40, 0, 700)
            T, P = rand_table(rng, 12), rand_struct_pssm(rng, 12)
            want_seq, want_st = oracle.stream_seq(s.codes, T), oracle.stream_struct(s.profile, P)
            fs, ft = want_seq[np.isfinite(want_seq)], want_st[np.isfinite(want_st)]
            has_seq, has_st = kind != "hits_dev_struct", kind != "hits_dev_letters"
            q_seq = {"hits_dev_letters": 0.9, "hits_dev_both": 0.7, "hits_adaptive_dev": 0.95}.get(kind)
            thr_seq = float(np.quantile(fs, q_seq)) if has_seq else -np.inf
            thr_st = float(np.quantile(ft, 0.9 if kind == "hits_dev_struct" else 0.3)) if has_st else -np.inf
            mo = ctx.motif(T if has_seq else None, P if has_st else None)
            self.motifs.append(mo)
            self.n_pos = s.n_pos
            self.want_pos = oracle.stream_hits(want_seq if has_seq else None, want_st if has_st else None, thr_seq, thr_st)
            self.seq_scores = want_seq if has_seq else None
            self.struct = (s.profile, P) if has_st else None
            codes, prof = torch.from_numpy(s.codes).to(DEV), torch.from_numpy(s.profile).to(DEV)
            self.keep = (codes, prof)
            if kind == "hits_adaptive_dev":
                # the two-phase route: the letters pass's candidates fit one candidate shard (1024 slots at this size)
                assert int((want_seq > thr_seq).sum()) < 1024
            f = ctx.hits_adaptive_dev if kind == "hits_adaptive_dev" else ctx.hits_dev

            def run(n_pos, cap, pos, seq, st, count):
                f(mo, codes.data_ptr() if has_seq else None, prof.data_ptr() if has_st else None, _lib.PROFILE_F32, n_pos,
                  thr_seq, thr_st, cap, pos, seq, st, count)
        elif kind == "hits_letters_f64_dev":
            s = letter_stream(rng, [int(x) for x in rng.integers(0, 701, size=40)])
            T = letter_table(rng, 8)
            mo = ctx.motif(T, None)
            self.motifs.append(mo)
            full = oracle.stream_letters_f64(s.codes, T)
            thr = _between(full, 0.9)
            self.n_pos, self.exact = s.n_pos, full
            self.want_pos = oracle.stream_hits(None, full, -np.inf, thr)
            codes = torch.from_numpy(s.codes).to(DEV)
            self.keep = (codes,)

            def run(n_pos, cap, pos, seq, st, count):
                ctx.hits_letters_f64_dev(mo, codes.data_ptr(), n_pos, thr, cap, pos, st, count)
        else:
            a, b = _pair_stream(rng, [int(x) for x in rng.integers(0, 701, size=40)])
            T, ST = rand_table(rng, 12), letter_table(rng, 12)
            ms, mt = ctx.motif(T, None), ctx.motif(ST, None)
            self.motifs += [ms, mt]
            fs, ft = oracle.stream_seq(a.codes, T), oracle.stream_letters_f64(b.codes, ST)
            thr_seq, thr_st = float(np.quantile(fs[np.isfinite(fs)], 0.8)) + 1e-4, _between(ft, 0.5)
            self.n_pos, self.seq_scores, self.exact = a.codes.size, fs, ft
            self.want_pos = oracle.stream_hits(fs, ft, thr_seq, thr_st)
            c1, c2 = torch.from_numpy(a.codes).to(DEV), torch.from_numpy(b.codes).to(DEV)
            self.keep = (c1, c2)

            def run(n_pos, cap, pos, seq, st, count):
                ctx.hits_pair_dev(ms, mt, c1.data_ptr(), c2.data_ptr(), n_pos, thr_seq, thr_st, cap, pos, seq, st, count)
        self.run = run

    def close(self):
        for mo in self.motifs:
            mo.close()


CAPACITY_KINDS = ["hits_dev_letters", "hits_dev_struct", "hits_dev_both", "hits_adaptive_dev", "hits_letters_f64_dev", "hits_pair_dev"]
FILL = 0x5A                                               # every byte of a hit array before the call


def _filled(n, dtype):
    import torch
    return torch.full((n * torch.empty((), dtype=dtype).element_size(),), FILL, dtype=torch.uint8, device=DEV).view(dtype)


@pytest.mark.parametrize("kind", CAPACITY_KINDS)
def test_capacity_below_the_hit_count(kind, ctx, oracle):
    import torch
    c = _Capacity(kind, ctx, oracle)
    try:
        k = len(c.want_pos)
        assert k >= 300
        cap = k // 3
        pos, seq, st = _filled(cap + 64, torch.int64), _filled(cap + 64, torch.float32), _filled(cap + 64, torch.float64)
        count = torch.zeros(1, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        c.run(c.n_pos, cap, pos.data_ptr(), seq.data_ptr(), st.data_ptr(), count.data_ptr())
        ctx.synchronize()
        assert int(count.item()) == k                     # the TOTAL, although only `cap` are stored
        got = pos[:cap].cpu().numpy()
        assert np.unique(got).size == cap and np.isin(got, c.want_pos).all()
        if c.seq_scores is not None:
            assert_f32_bits_equal(seq[:cap].cpu().numpy(), c.seq_scores[got])
        if c.struct is not None:
            assert_struct_tight(st[:cap].cpu().numpy(), c.struct[0], c.struct[1], positions=got)
        if c.exact is not None:
            assert np.array_equal(st[:cap].cpu().numpy(), c.exact[got])
        for name, arr in (("hit_pos", pos), ("hit_seq", seq), ("hit_struct", st)):
            tail = arr[cap:].view(torch.uint8).cpu().numpy()
            assert (tail == FILL).all(), "%s: %d bytes written behind capacity" % (name, int((tail != FILL).sum()))
        if c.seq_scores is None:                          # a side the motif does not have is not written at all
            assert bool((seq.view(torch.uint8) == FILL).all())
        if c.struct is None and c.exact is None:
            assert bool((st.view(torch.uint8) == FILL).all())
        # capacity 0 with no hit arrays: the count alone
        count.zero_()
        torch.cuda.synchronize()
        c.run(c.n_pos, 0, None, None, None, count.data_ptr())
        ctx.synchronize()
        assert int(count.item()) == k
        # an empty stream: the count stays as it was, nothing is written
        count.fill_(777)
        keep = (pos.clone(), seq.clone(), st.clone())
        torch.cuda.synchronize()
        c.run(0, cap, pos.data_ptr(), seq.data_ptr(), st.data_ptr(), count.data_ptr())
        ctx.synchronize()
        assert int(count.item()) == 777
        for a, b in zip(keep, (pos, seq, st)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    finally:
        c.close()
