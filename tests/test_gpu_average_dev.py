"""pfmscan_average_dev as an integrator calls it: annotated letters, fragment / record tables and the value table in the
caller's own device buffers (torch tensors), a caller-chosen max_len, tables that rnascan_amd.average never builds.

The reference is plain numpy: per output row the letters of every fragment that covers it are counted (a code >= 7 counts
for nothing), the row is T[n (n + 1) / 2 + c] per column for its coverage n and counts c, a zero row follows each record;
rows are compared bit for bit in float64 and in float32 (the round-to-nearest cast).  Every verdict of the header is
produced -- AVG_COVER, AVG_UNCOVERED, and AVG_BAD_TABLE once per clause of k_avg_check -- with tables that stay inside the
buffers handed over, and after each rejection the same context averages a valid set correctly.  Every test opens its own
context."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_LEN = 150          # the longest fragment of the random sets
N_MAX = 64             # the largest coverage the value table of these tests holds
PAD = 1024             # letters behind the last fragment: a fragment table that over-runs its record still reads the caller's buffer
TABLE_NAMES = ("letters", "frag_off", "frag_len", "frag_row", "rec_row", "rec_len", "rec_frag")


@pytest.fixture
def own_ctx():
    from rnascan_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def value_table(n_max=N_MAX):
    from rnascan_amd import average
    return np.array(average.value_table(n_max))


# ---- sets and tables ----------------------------------------------------------------------------------------------------
def random_set(rng, n_rec=40):
    """records [(length, [(first row inside the record, letters uint8)])]: every row covered by a letter 0..6, further
    fragments with codes >= 7 among their letters, starts in any order; record lengths on the wave (64) and workgroup (256)
    edges, a record of one row, a fragment of MAX_LEN letters, a fragment that ends exactly ON the first row of a wave
    (start = row0 - MAX_LEN + 1) and one that starts on a wave's last row (row0 + 63), a record whose rows are covered
    exactly N_MAX times"""
    edges = [1, 63, 64, 65, 255, 256, 257]
    recs = []
    for r in range(n_rec):
        if r == 0:
            L = 1000                                      # its rows are rows 0..999 of the output: wave w starts at row 64 w
        elif r % 3 == 1:
            L = edges[(r // 3) % len(edges)]
        else:
            L = int(rng.integers(1, 600))
        frags, at = [], 0
        while at < L:                                     # a chain of fragments of letters 0..6 that covers every row
            s = at - int(rng.integers(0, min(at, 20) + 1))
            n = min(int(rng.integers(at - s + 1, at - s + 1 + 60)), L - s, MAX_LEN)
            frags.append((s, rng.integers(0, 7, size=n).astype(np.uint8)))
            at = s + n
        for _ in range(int(rng.integers(0, 12))):         # others, some of their codes foreign (7, lower-case bit, a large byte)
            s = int(rng.integers(0, L))
            n = min(int(rng.integers(1, MAX_LEN + 1)), L - s)
            c = rng.integers(0, 7, size=n).astype(np.uint8)
            c[rng.random(n) < 0.1] = rng.choice(np.array([7, 8, 15, 200], dtype=np.uint8))
            frags.append((s, c))
        if r == 0:
            row0 = 512
            frags.append((row0 - MAX_LEN + 1, rng.integers(0, 7, size=MAX_LEN).astype(np.uint8)))     # its last letter is row0's
            frags.append((row0 + 63, rng.integers(0, 7, size=10).astype(np.uint8)))                   # starts on the wave's last row
        order = rng.permutation(len(frags))
        recs.append((L, [frags[k] for k in order]))
    deep = (9, [(0, rng.integers(0, 7, size=9).astype(np.uint8)) for _ in range(N_MAX)])               # coverage N_MAX, every row
    recs.insert(n_rec // 2, deep)
    return recs


def build_tables(recs):
    """-> dict of the arrays pfmscan_average_dev takes (fragments sorted by record, then by row), n_rows, the longest fragment"""
    letters, frag_off, frag_len, frag_row, rec_row, rec_len, rec_frag = [], [], [], [], [], [], [0]
    at, row = 0, 0
    for L, frags in recs:
        rec_row.append(row)
        rec_len.append(L)
        for s, c in sorted(frags, key=lambda f: f[0]):
            assert 0 <= s and s + len(c) <= L and len(c) >= 1
            frag_off.append(at)
            frag_len.append(len(c))
            frag_row.append(row + s)
            letters.append(c)
            letters.append(np.array([7], dtype=np.uint8))
            at += len(c) + 1
        rec_frag.append(len(frag_off))
        row += L + 1
    letters.append(np.full(PAD, 7, dtype=np.uint8))
    t = {"letters": np.concatenate(letters) if letters else np.zeros(0, np.uint8)}
    for name, v in zip(TABLE_NAMES[1:], (frag_off, frag_len, frag_row, rec_row, rec_len, rec_frag)):
        t[name] = np.array(v, dtype=np.int64)
    return t, row, int(max(frag_len)) if frag_len else 1


def want_rows(recs, T, dtype):
    rows = []
    for L, frags in recs:
        cnt = np.zeros((L, 7), dtype=np.int64)
        for s, c in frags:
            keep = c < 7
            np.add.at(cnt, (np.arange(s, s + len(c))[keep], c[keep].astype(np.int64)), 1)
        n = cnt.sum(axis=1)
        assert (n > 0).all() and n.max() <= N_MAX
        rows.append(T[(n * (n + 1) // 2)[:, None] + cnt])
        rows.append(np.zeros((1, 7)))
    return np.concatenate(rows).astype(dtype)


def to_device(t, T):
    import torch
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for k, v in t.items()}
    d["table"] = torch.from_numpy(np.ascontiguousarray(T)).to("cuda:0")
    return d


def call_average(ctx, d, n_rows, max_len, out, dtype, n_max=N_MAX, stream=None):
    """pfmscan_average_dev on the device tensors of `d` (the table sizes are the tensors' sizes)"""
    ctx.average_dev(d["letters"], d["letters"].numel(), d["frag_off"], d["frag_len"], d["frag_row"],
                    d["frag_off"].numel(), max_len, d["rec_row"], d["rec_len"], d["rec_frag"],
                    d["rec_row"].numel(), n_rows, d["table"], n_max, out, dtype=dtype, stream=stream)


def average(ctx, t, T, n_rows, max_len, dtype):
    import torch
    d = to_device(t, T)
    out = torch.full((n_rows, 7), -7.0, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    call_average(ctx, d, n_rows, max_len, out, dtype)
    ctx.synchronize()
    return out.cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. random sets ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_random_sets_equal_the_numpy_reference(own_ctx, dtype):
    rng = np.random.default_rng(31 if dtype == np.float64 else 32)
    recs = random_set(rng)
    t, n_rows, longest = build_tables(recs)
    assert longest == MAX_LEN and 1 in [L for L, _ in recs]
    row0 = 512                                            # record 0 starts at row 0: the two fragments on a wave's edges are there
    assert row0 % 64 == 0 and (row0 - MAX_LEN + 1) in t["frag_row"] and (row0 + 63) in t["frag_row"]
    T = value_table()
    want = want_rows(recs, T, dtype)
    got = average(own_ctx, t, T, n_rows, longest, dtype)
    assert same_bits(got, want), np.flatnonzero((got != want).any(axis=1))[:10]
    # a caller that only knows a bound on the fragment length: the same rows
    again = average(own_ctx, t, T, n_rows, 4 * longest, dtype)
    assert same_bits(again, want), np.flatnonzero((again != want).any(axis=1))[:10]


def test_no_records_is_ok_and_writes_nothing(own_ctx):
    import torch
    t, n_rows, _ = build_tables([])
    assert n_rows == 0
    d = to_device(t, value_table())
    out = torch.full((4, 7), -7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    call_average(own_ctx, d, 0, 1, out, np.float64)
    own_ctx.synchronize()
    assert bool((out == -7.0).all())


# ---- 2. verdicts ---------------------------------------------------------------------------------------------------------
def _valid_set():
    rng = np.random.default_rng(77)
    recs = random_set(rng, 24)
    t, n_rows, longest = build_tables(recs)
    return recs, t, n_rows, longest


def _rejected(ctx, t, T, n_rows, max_len):
    import torch
    d = to_device(t, T)
    out = torch.zeros((n_rows, 7), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(ValueError) as e:
        call_average(ctx, d, n_rows, max_len, out, np.float64)
    ctx.synchronize()
    return e.value.kind, e.value.position


def _recovers(ctx, recs, t, T, n_rows, longest):
    got = average(ctx, t, T, n_rows, longest, np.float64)
    assert same_bits(got, want_rows(recs, T, np.float64))


def test_a_row_covered_once_too_often(own_ctx):
    from rnascan_amd import _lib
    recs, t, n_rows, longest = _valid_set()
    T = value_table()
    deep = [r for r, (L, frags) in enumerate(recs) if len(frags) == N_MAX and L == 9][0]
    bad = list(recs)
    bad[deep] = (9, recs[deep][1] + [(3, np.zeros(4, dtype=np.uint8))])                  # rows 3..6 of it: N_MAX + 1 times
    bt, bn, bl = build_tables(bad)
    kind, at = _rejected(own_ctx, bt, T, bn, bl)
    assert (kind, at) == (_lib.AVG_COVER, int(bt["rec_row"][deep]) + 3)
    _recovers(own_ctx, recs, t, T, n_rows, longest)


@pytest.mark.parametrize("how", ["foreign_codes_only", "no_fragment"])
def test_an_uncovered_row(own_ctx, how):
    from rnascan_amd import _lib
    recs, t, n_rows, longest = _valid_set()
    T = value_table()
    L = 40
    if how == "foreign_codes_only":                       # rows 11, 12 and 30 are covered, but by codes that count for nothing
        c = np.arange(L, dtype=np.uint8) % 7
        c[[11, 12, 30]] = [7, 9, 255]
        frags = [(0, c)]
        first = 11
    else:                                                 # rows 17..24 lie between two fragments
        frags = [(25, np.ones(15, dtype=np.uint8)), (0, np.ones(17, dtype=np.uint8))]
        first = 17
    bad = list(recs)
    at_rec = 5
    bad.insert(at_rec, (L, frags))
    bt, bn, bl = build_tables(bad)
    kind, at = _rejected(own_ctx, bt, T, bn, bl)
    assert (kind, at) == (_lib.AVG_UNCOVERED, int(bt["rec_row"][at_rec]) + first)
    _recovers(own_ctx, recs, t, T, n_rows, longest)


CLAUSES = ["rows_not_contiguous", "starts_not_sorted", "fragment_past_record_end", "frag_len_zero", "frag_len_above_max_len"]


@pytest.mark.parametrize("which", ["first_record", "a_later_record"])
@pytest.mark.parametrize("clause", CLAUSES)
def test_bad_table_names_the_record(own_ctx, clause, which):
    """one clause of k_avg_check per case, broken in record 0 -- where the record's index is as small as the index of the rows
    the broken table leaves uncovered -- and in a later record; every index stays inside the arrays handed over"""
    from rnascan_amd import _lib
    recs, t, n_rows, longest = _valid_set()
    T = value_table()
    long_ones = [r for r, (L, _) in enumerate(recs) if r > 0 and L >= 2 * MAX_LEN + 2]
    r = 0 if which == "first_record" else long_ones[0]
    bt = {k: v.copy() for k, v in t.items()}
    f0, f1 = int(t["rec_frag"][r]), int(t["rec_frag"][r + 1])
    max_len = longest
    if clause == "rows_not_contiguous":
        bt["rec_row"][r] += 1
    elif clause == "starts_not_sorted":
        a = f0
        b = a + 1 + int(np.flatnonzero(t["frag_row"][a + 1:f1] > t["frag_row"][a])[0])          # a fragment that starts later
        for name in ("frag_off", "frag_len", "frag_row"):
            bt[name][[a, b]] = t[name][[b, a]]
    elif clause == "fragment_past_record_end":
        f = f1 - 1                                        # the fragment with the largest start
        end = int(t["rec_row"][r] + t["rec_len"][r])
        bt["frag_len"][f] = end - int(t["frag_row"][f]) + 1                                     # one row past the end
        max_len = 4 * longest
        assert bt["frag_len"][f] <= max_len and bt["frag_off"][f] + bt["frag_len"][f] <= t["letters"].size
    elif clause == "frag_len_zero":
        bt["frag_len"][f0] = 0                            # the first fragment: row 0 of the record may now be uncovered, too
    elif clause == "frag_len_above_max_len":
        assert t["frag_row"][f0] == t["rec_row"][r]       # starts at the record's first row, which is long enough for it
        bt["frag_len"][f0] = longest + 1
        assert bt["frag_off"][f0] + longest + 1 <= t["letters"].size
    kind, at = _rejected(own_ctx, bt, T, n_rows, max_len)
    assert (kind, at) == (_lib.AVG_BAD_TABLE, r)
    _recovers(own_ctx, recs, t, T, n_rows, longest)


def test_bad_table_rec_frag_not_ending_at_n_frag(own_ctx):
    from rnascan_amd import _lib
    recs, t, n_rows, longest = _valid_set()
    T = value_table()
    bt = {k: v.copy() for k, v in t.items()}
    bt["rec_frag"][-1] -= 1                               # the last record leaves the last fragment out
    kind, at = _rejected(own_ctx, bt, T, n_rows, longest)
    assert (kind, at) == (_lib.AVG_BAD_TABLE, len(recs) - 1)
    _recovers(own_ctx, recs, t, T, n_rows, longest)
