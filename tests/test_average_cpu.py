"""Fragment averaging, host side: the windows against the reference's Python 2 arithmetic, fragment ids, the RNAfold
reader, the value table against pandas itself, and the numpy restatement against the reference's own output
(tests/golden/average/, made by tests/golden/make_average_golden.py)."""
import io

import numpy as np
import pytest

from average_rules import PAIRS, counts, golden, py2_starts, split_name, text
from dotbracket_rules import annotate


def test_windows_are_python2_range():
    from rnascan_amd import average
    L = np.arange(1, 401)
    for w in range(2, 131):
        for o in range(w):
            rec, start = average.window_starts(L, w, o)
            cut = np.searchsorted(rec, np.arange(L.size + 1))
            for l in (1, 2, 3, w // 2, w // 2 + 1, w - 1, w, w + 1, 2 * w + 3, 137, 400):
                if l > 400:
                    continue
                got = start[cut[l - 1]:cut[l]].tolist()
                assert got == py2_starts(l, w, o), (w, o, l)
    # every length once for a few pairs
    for w, o in ((100, 95), (40, 30), (101, 0), (7, 3), (2, 1), (3, 0)):
        rec, start = average.window_starts(L, w, o)
        want = [s for l in L.tolist() for s in py2_starts(l, w, o)]
        assert start.tolist() == want
        assert rec.tolist() == [r for r, l in enumerate(L.tolist()) for _ in py2_starts(l, w, o)]


def test_hand_case_l120():
    from rnascan_amd import average
    _, start = average.window_starts([120], 100, 95)
    assert start.size == 24
    assert (max(start[0], 0), min(start[0] + 100, 120)) == (0, 50)
    assert (max(start[-1], 0), min(start[-1] + 100, 120)) == (65, 120)


def test_window_arguments_are_checked():
    from rnascan_amd import average
    for w, o in ((1, 0), (0, 0), (10, 10), (10, -1), (10, 11)):
        with pytest.raises(ValueError):
            average.check_window(w, o)


def test_fragments_skip_short_records(tmp_path):
    from rnascan_amd import average
    p = tmp_path / "s.fa"
    p.write_text(">fifty\n" + "A" * 50 + "\n>fiftyone\n" + "acgT" * 12 + "ACG\n>tiny\nAC\n")
    out = b"".join(average.fragments_fasta(str(p))).decode()
    names = [l[1:] for l in out.split("\n") if l.startswith(">")]
    assert names == ["fiftyone_frag_%d" % i for i in py2_starts(51, 100, 95)]
    body = out.split("\n")[1]
    assert body == ("acgT" * 12 + "ACG")[:50]                   # as given: no case or U/T change


def test_fragment_ids():
    from rnascan_amd import _lib
    ids = [b"a_frag_-50", b"x_frag_y_frag_5", b"rec_frag_0", b"a_frag_", b"a_frag_x", b"a", b"_frag_3", b"a_frag_1 "]
    buf = b" ".join(ids)
    spans, at = [], 0
    for i in ids:
        spans.append((at, len(i)))
        at += len(i) + 1
    arr = np.frombuffer(buf, dtype=np.uint8)
    key_len, start = _lib.fragment_ids(arr, np.array(spans[:3]))
    assert key_len.tolist() == [1, 8, 3] and start.tolist() == [-50, 5, 0]
    for k in range(3, len(ids)):
        with pytest.raises(ValueError) as e:
            _lib.fragment_ids(arr, np.array(spans[:3] + [spans[k]]))
        assert e.value.index == 3


RNAFOLD = """>r1_frag_-2
GGGAAAUCCA
(((...))). ( -1.20)
(((...))), [ -1.50]
(((...))). { -1.20 d=1.50}
 frequency of mfe structure in ensemble 0.5; ensemble diversity 1.20
>r1_frag_2
GAAAUCCA
.(....). ( -0.20)
.(....)., [ -0.50]
........ {  0.00 d=1.00}
 frequency of mfe structure in ensemble 0.4; ensemble diversity 1.00
"""


def test_rnafold_reader(tmp_path):
    from rnascan_amd import average
    p = tmp_path / "fold.txt"
    p.write_text(RNAFOLD)
    fr = average.Fragments(str(p), "rnafold")
    assert fr.ids == ["r1"] and fr.start.tolist() == [-2, 2] and fr.flen.tolist() == [10, 8]
    assert fr.lengths.tolist() == [10]
    codes, offsets = fr.encode(0, 2)
    from rnascan_amd import dotbracket
    want = [dotbracket.LUT[np.frombuffer(s.encode(), dtype=np.uint8)] for s in ("(((...))).", "........")]
    assert offsets.tolist() == [0, 11] and codes[:10].tolist() == want[0].tolist() and codes[10] == 7
    assert codes[11:19].tolist() == want[1].tolist() and codes[19] == 7 and codes.size == 20
    bad = tmp_path / "bad.txt"
    bad.write_text(RNAFOLD.replace("........ {", "....... {"))
    with pytest.raises(average.AverageError) as e:
        average.Fragments(str(bad), "rnafold")
    assert "r1_frag_2" in str(e.value) and str(bad) in str(e.value)
    cut = tmp_path / "cut.txt"
    cut.write_text("\n".join(RNAFOLD.split("\n")[:9]) + "\n")
    with pytest.raises(average.AverageError) as e:
        average.Fragments(str(cut), "rnafold")
    assert "r1_frag_2" in str(e.value) and "truncated" in str(e.value)


def test_fasta_fragments_grouping(tmp_path):
    from rnascan_amd import average
    p = tmp_path / "f.fa"
    p.write_text(">b_frag_4\n..\n>b_frag_0\n(..)\n>a_frag_-1\n...\n>b_frag_2\n.\n")
    with pytest.raises(average.AverageError) as e:
        average.Fragments(str(p))
    assert "'b'" in str(e.value) and "contiguous" in str(e.value) and str(p) in str(e.value)
    p.write_text(">b_frag_4\n..\n>b_frag_0\n(..)\n>a_frag_-1\n...\n>a_frag_1\n.\n")
    fr = average.Fragments(str(p))
    assert fr.ids == ["b", "a"] and fr.lengths.tolist() == [6, 3] and fr.rec_frag.tolist() == [0, 2, 4]
    p.write_text(">b_frag_4\n..\n>b_fra_0\n(..)\n")
    with pytest.raises(average.AverageError) as e:
        average.Fragments(str(p))
    assert "b_fra_0" in str(e.value) and str(p) in str(e.value)


def test_value_table_is_what_pandas_reads():
    import pandas as pd
    from rnascan_amd import average
    T = average.value_table(64)
    c, n = average._triangle(64)
    src = "x\n" + "".join("%r\n" % (float(a) / float(b)) for a, b in zip(c[1:].tolist(), n[1:].tolist()))
    want = pd.read_table(io.StringIO(src))["x"].to_numpy(dtype=np.float64)
    assert np.array_equal(T[1:].view(np.int64), want.view(np.int64))
    assert np.any(T[1:] != c[1:] / n[1:])                       # the reason the table exists
    E = average.value_table(64, exact=True)
    assert np.array_equal(E[1:], c[1:] / n[1:])


@pytest.mark.parametrize("w,o", PAIRS)
def test_restatement_reproduces_the_reference(w, o):
    seqs, frags, texts = golden(w, o)
    by_rec = {}
    for name, s in frags:
        key, i = split_name(name)
        by_rec.setdefault(key, []).append((max(i, 0), annotate(s)))
    assert len(texts) == len(by_rec) > 0
    for key, fr in by_rec.items():
        got = text(counts([p for p, _ in fr], [s for _, s in fr]))
        assert got == texts["structure.%s.txt" % key], key
    # the fragments are run_folding's windows of the golden sequences
    seq = dict(seqs)
    for key, fr in by_rec.items():
        names = [n for n, _ in frags if split_name(n)[0] == key]
        assert [split_name(n)[1] for n in names] == py2_starts(len(seq[key]), w, o)
