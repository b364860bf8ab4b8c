"""The dot-bracket annotation rules restated in plain Python (a test helper, no device).

One record ``s`` over ``(``, ``)``, ``.``, balanced.  ``p[i]`` is the partner of bracket ``i``; ``depth(i)`` is the number
of ``(`` before ``i`` minus the number of ``)`` before ``i``.

1. ``(`` -> L, ``)`` -> R.
2. Every maximal run of dots ``[a, b)`` gets one label; ``k = a - 1``, ``m = b``:
   5' or 3' tail (``k < 0`` or ``m == n``) -> E;  ``(`` .. ``)`` -> H;  ``)`` .. ``(`` -> M if ``depth(a) > 0`` else E;
   both ``(`` or both ``)`` -> B if ``p[m] + 1 == p[k]``, else provisional N.
3. For every ``j`` with ``s[j] == ')'``, ``j + 1 < n`` and step-2 label L or M at ``j + 1``: with ``m`` the first bracket
   at or after ``j + 1`` (a ``(``), every N of the dot run ending at ``p[j] - 1`` and of the dot run starting at
   ``p[m] + 1`` becomes M.
4. Every remaining N -> T.

The committed fixtures under tests/golden/dotbracket/ (the reference parser's output) pin this restatement; the device
kernels are tested against it.
"""
import numpy as np


def partners(s):
    """partner of every bracket (-1 for dots); ValueError on anything but a balanced ``().`` string"""
    p = [-1] * len(s)
    stack = []
    for i, c in enumerate(s):
        if c == "(":
            stack.append(i)
        elif c == ")":
            if not stack:
                raise ValueError("unbalanced ')' at %d" % i)
            j = stack.pop()
            p[i], p[j] = j, i
        elif c != ".":
            raise ValueError("character %r at %d" % (c, i))
    if stack:
        raise ValueError("unbalanced '(' at %d" % stack[-1])
    return p


def annotate(s):
    """dot-bracket string -> structure-context letters (EHTBLRM), the rules above"""
    n = len(s)
    p = partners(s)
    lab = ["L" if c == "(" else "R" if c == ")" else None for c in s]
    run_of = {}                                   # dot position -> (a, b) of its run
    depth = 0
    a = 0
    while a < n:
        if s[a] != ".":
            depth += 1 if s[a] == "(" else -1
            a += 1
            continue
        b = a
        while b < n and s[b] == ".":
            b += 1
        k, m = a - 1, b
        if k < 0 or m == n:
            x = "E"
        elif s[k] == "(" and s[m] == ")":
            x = "H"
        elif s[k] == ")" and s[m] == "(":
            x = "M" if depth > 0 else "E"
        else:
            x = "B" if p[m] + 1 == p[k] else "N"
        for i in range(a, b):
            lab[i] = x
            run_of[i] = (a, b)
        a = b
    step2 = list(lab)

    def relabel(i):
        if 0 <= i < n and s[i] == ".":
            ra, rb = run_of[i]
            for t in range(ra, rb):
                if lab[t] == "N":
                    lab[t] = "M"

    for j in range(n - 1):
        if s[j] == ")" and step2[j + 1] in ("L", "M"):
            m = j + 1
            while s[m] == ".":
                m += 1
            relabel(p[j] - 1)                     # the run ending at p[j] - 1
            relabel(p[m] + 1)                     # the run starting at p[m] + 1
    return "".join("T" if x == "N" else x for x in lab)


def random_structure(rng, n, p_pair=None):
    """a balanced dot-bracket string of length n with stems, hairpins, bulges, interior loops and multiloops: a random
    walk that opens stems of 1..12 pairs, leaves runs of 0..8 unpaired bases and closes what is open when the remaining
    length asks for it"""
    p_pair = rng.uniform(0.2, 0.8) if p_pair is None else p_pair
    out = []
    open_ = 0
    while len(out) < n:
        left = n - len(out)
        if open_ >= left:                         # must close everything now
            out.append(")")
            open_ -= 1
            continue
        r = rng.random()
        if r < p_pair * 0.5 and left - open_ >= 2:
            stem = int(min(rng.integers(1, 13), (left - open_) // 2))
            out.extend("(" * stem)
            open_ += stem
        elif r < p_pair and open_ > 0 and out and out[-1] != "(":
            stem = int(min(rng.integers(1, 13), open_))
            out.extend(")" * stem)
            open_ -= stem
        else:
            run = int(min(rng.integers(1, 9), left - open_))
            out.extend("." * max(run, 1))
    assert open_ == 0 and len(out) == n          # a stem opens only what the remaining length can close
    return "".join(out)


def deep_structure(depth, n_dots_inside=3, tail=0):
    """one stem of ``depth`` nested pairs around a hairpin: depth ``depth``, the outermost pair spans 2*depth + dots"""
    return "(" * depth + "." * n_dots_inside + ")" * depth + "." * tail


def count_letters(letters, alphabet="EHTBLRM"):
    """int64 [7] occurrences of each alphabet letter in a string"""
    b = np.frombuffer(letters.encode("ascii"), dtype=np.uint8)
    c = np.bincount(b, minlength=256)
    return np.array([c[ord(x)] for x in alphabet], dtype=np.int64)
