"""TEST-ONLY helpers of the profile-background tests (CPU and GPU): the oracle-backed engine whose ``profile_colsums`` is
the numpy restatement (tests/background_rules.py), writers of small inputs, and a stand-in for a process group."""
import pickle

import numpy as np

import background_rules as rules
from engines import OracleEngine

COLUMNS = "BEHLMRT"


class RulesEngine(OracleEngine):
    """the oracle-backed engine + profile_colsums from the restated rules (same contract as HipEngine.profile_colsums)"""

    def profile_colsums(self, stream):
        bad = rules.first_bad(stream.profile, stream.offsets, stream.lengths)
        if bad >= 0:
            err = ValueError("bad cell")
            err.element = bad
            raise err
        return rules.colsums(stream.profile, stream.offsets, stream.lengths)


def one_hot(s, columns=COLUMNS):
    p = np.zeros((len(s), 7), dtype=np.float64)
    for i, ch in enumerate(s):
        p[i, columns.index(ch)] = 1.0
    return p


def write_profile(path, prof, columns=COLUMNS, fmt=repr):
    with open(path, "w") as f:
        f.write("PO\t" + "\t".join(columns) + "\n")
        for i, row in enumerate(np.asarray(prof).tolist()):
            f.write(str(i) + "".join("\t" + (x if isinstance(x, str) else fmt(x)) for x in row) + "\n")


def write_fasta(path, records):
    with open(path, "w") as f:
        for rid, s in records:
            f.write(">%s\n%s\n" % (rid, s))


def random_rows(rng, L):
    """non-negative rows that sum to 1, cells multiples of 1/1024"""
    cut = np.sort(rng.integers(0, 1025, size=(L, 6)), axis=1)
    edges = np.concatenate([np.zeros((L, 1), dtype=np.int64), cut, np.full((L, 1), 1024)], axis=1)
    return np.diff(edges, axis=1) / 1024.0


class _Sent(Exception):
    pass


class FakeDist(object):
    """all_gather_object of ``world`` ranks that run one after the other in this process: without ``payloads`` it keeps
    what the rank sends (pickled, as a process group would) and stops the rank; with them it hands them out"""

    def __init__(self, payloads=None):
        self.payloads, self.sent = payloads, None

    def all_gather_object(self, out, obj):
        if self.payloads is None:
            self.sent = pickle.dumps(obj)
            raise _Sent()
        for i, p in enumerate(self.payloads):
            out[i] = pickle.loads(p)


def as_ranks(world, fn):
    """fn(rank, world, dist) as every rank of ``world`` would run it -> per rank its result, or the exception it raised"""
    payloads = []
    for rank in range(world):
        d = FakeDist()
        try:
            fn(rank, world, d)
        except _Sent:
            pass
        payloads.append(d.sent)
    out = []
    for rank in range(world):
        try:
            out.append(fn(rank, world, FakeDist(payloads)))
        except Exception as e:
            out.append(e)
    return out
