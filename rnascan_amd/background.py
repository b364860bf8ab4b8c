"""Structure background of an averaged-structure input (profile directory, packed store, averaged fragments).

The reference computes a background from FASTA records only (``compute_background``, rnascan.py:440-465): letter counts
with a +1 pseudocount per letter.  ``load_background`` (:468-484) hands it whatever the structure input is, so its
fourth mode (``rnascan -p .. -q .. seqs.fa averaged_structures/``) has no default background.  For a profile the count of
letter c is the expected number of that letter:

    count[c]   = sum over every row of every record of column c
    total      = 7 + sum over c of count[c]
    content[c] = (count[c] + 1) / total          for c in "EHTBLRM", in that order

then the reference's low-content warning, stderr lines and sum assertion, unchanged.  Columns are matched to letters by
NAME (the file header / the store's index).  For one-hot rows this is ``compute_background`` of the letter strings,
number for number.

The sums are made on the GPU per RECORD (``HipEngine.profile_colsums``: a fixed order of additions inside a record, see
include/pfmscan.h) and the records are combined here with ``math.fsum``, which is exactly rounded: the dict has the same
bits whatever the batch size, the pipeline chunk, the upload mode, the input form and the number of ranks.
"""
import math
import os
import warnings

import numpy as np

from . import fasta, pack, shard, store

# records per launch set of a store, in units of RNASCAN_BATCH_POSITIONS.  Any bound would do: the result does not depend
# on it, and the device scratch is bounded by pfmscan_profile_colsums_host's own pieces (PFMSCAN_COLSUMS_CHUNK) anyway.
STORE_BATCHES = 32


class BackgroundError(ValueError):
    """a cell from which no background can be computed; ``record``, ``position`` (1-based) and ``letter`` say where"""

    def __init__(self, record, position, letter, value):
        ValueError.__init__(self, "Averaged-structure profile %s holds %r at position %d, column %s: no background can be "
                                  "computed from it (fix the profile, or give -u or -B)" % (record, value, position, letter))
        self.record, self.position, self.letter, self.value = record, position, letter, value

    def __reduce__(self):            # ranks hand it to each other (record_sums): rebuilt from its four fields
        return (BackgroundError, (self.record, self.position, self.letter, self.value))


class InputError(ValueError):
    """an averaged-structure input no background can be read from (the message says which file and why)"""


def _batch_sums(engine, stream, ids, letters_of):
    """letters_of(record index in the batch) -> that record's column letters"""
    try:
        return engine.profile_colsums(stream)
    except ValueError as e:
        at = getattr(e, "element", None)
        if at is None:
            raise
        row, col = divmod(int(at), 7)
        rec, start = stream.locate(np.asarray([row]))
        rec = int(rec[0])
        raise BackgroundError(ids[rec], int(start[0]) + 1, letters_of(rec)[col], float(stream.profile[row, col]))


def _portable(e):
    """an exception another rank can rebuild"""
    import pickle
    try:
        pickle.loads(pickle.dumps(e))
        return e
    except Exception:
        return RuntimeError("%s: %s" % (type(e).__name__, e))


def record_sums(engine, source, rank=0, world=1, dist=None):
    """(ids, column letters, float64 [n_records][7]) of EVERY record of ``source`` -- a directory of structure.<id>.txt
    files or a packed store.  A record's row is its structural composition: the expected number of each context letter.
    A store's rows come in the store's column order; the files of a directory may each have their own (the scan pairs
    them by name per file too), their rows come in ``pack.STRUCT_COLUMNS`` order.
    With several ranks each sums the records of its own share (shard.partition, as the scan shards them) and the rows
    are exchanged once over the process group, host side; a rank that fails hands its exception over instead, and
    every rank raises the one of the lowest rank (shares are contiguous and in rank order: for a rejected cell that is
    the earliest in input order)."""
    if store.is_store(source):
        ps = store.ProfileStore(source)
        ids, letters, lengths = ps.ids, list(ps.letters), ps.lengths

        def batch(a, b):
            return _batch_sums(engine, ps.stream(a, b), ids[a:b], lambda r: letters)
        max_positions = STORE_BATCHES * shard.batch_positions()
    else:
        files = fasta.list_profiles(source)
        if len(files) == 0:
            raise IOError("No averaged structure files found")
        ids = [sid for sid, _ in files]
        lengths = [os.path.getsize(path) // 64 + 1 for _, path in files]          # as cli.scan_main weighs them
        letters = list(pack.STRUCT_COLUMNS)

        def batch(a, b):
            parsed = fasta.read_profiles([path for _, path in files[a:b]])
            for (_, path), (file_letters, _) in zip(files[a:b], parsed):
                if sorted(file_letters) != sorted(letters):
                    raise InputError("%s: its columns %s are not the seven structure letters %s" %
                                     (path, list(file_letters), "".join(letters)))
            # the parsed float64 values ARE the input, whatever storage the scan picks for them (--profile-dtype)
            stream = pack.pack(profiles=[p for _, p in parsed], profile_dtype=np.float64)
            sums = _batch_sums(engine, stream, ids[a:b], lambda r: list(parsed[r][0]))
            for r, (file_letters, _) in enumerate(parsed):                        # columns are matched BY NAME, file by file
                if list(file_letters) != letters:
                    sums[r] = sums[r][[list(file_letters).index(c) for c in letters]]
            return sums
        max_positions = shard.batch_positions()
    lo, hi = shard.partition(lengths, world)[rank]
    mine, failure = [], None
    try:
        for a, b in (shard.batches(lengths, lo, hi, max_positions) if hi > lo else []):
            mine.append(batch(a, b))
    except Exception as e:
        if world == 1:
            raise
        failure = _portable(e)
    local = np.concatenate(mine) if mine else np.zeros((0, 7), dtype=np.float64)
    if world > 1:
        shares = [None] * world
        dist.all_gather_object(shares, (failure, None if failure is not None else local))
        for bad, _ in shares:
            if bad is not None:
                raise bad
        local = np.concatenate([s for _, s in shares])
    return ids, letters, local


def content_from_sums(sums, letters, verbose=True):
    """per-record column sums [n][7] + their column letters -> the background dict (module docstring)"""
    letters = list(letters)
    if sorted(letters) != sorted(fasta.STRUCT):
        raise ValueError("averaged-structure columns %s are not the letters %s" % (letters, fasta.STRUCT))
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 7)
    content = {}
    for letter in fasta.STRUCT:
        content[letter] = math.fsum(sums[:, letters.index(letter)].tolist())
    total = math.fsum([float(len(fasta.STRUCT))] + list(content.values()))
    pct_sum = 0.0
    for letter, count in content.items():
        content[letter] = (float(count) + 1) / total
        if content[letter] <= 0.05:
            warnings.warn("Letter %s has low content: %0.2f" % (letter, content[letter]), Warning)
        pct_sum += content[letter]
    if verbose:
        fasta.eprint(dict(content))
    assert abs(1.0 - pct_sum) < 0.0001, "Background sums to %f" % pct_sum
    return content


def profile_background(engine, source, rank=0, world=1, dist=None, verbose=True):
    """the structure background of an averaged-structure directory or packed store (module docstring); the same dict on
    every rank.  Raises BackgroundError for a NaN, infinite or negative cell (the earliest in input order)."""
    fasta.eprint("Calculating background probabilities...")
    _, letters, sums = record_sums(engine, source, rank, world, dist)
    return content_from_sums(sums, letters, verbose)
