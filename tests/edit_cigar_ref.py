"""The naive restatement of the base-level alignment of a mapping (metamaps_amd/csrc/mm_edit_core.hpp has the definition): d, a, b from
tests/edit_ref.py, then the whole suffix table E[i][j] = distance of Q[i, m) to T[j, n), T = window[a, b), one numpy row per read base, and the walk
from (0, 0) to (m, n) that takes = before X before I before D.  Runs are BAM's words: len << 4 | op with I = 1, D = 2, = = 7, X = 8."""
import numpy as np

import edit_ref

OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
LETTER = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}


def _suffix_table(q, t):
    """E as an (m + 1) x (n + 1) array: the anchored table of the reversed strings, turned round"""
    m, n = len(q), len(t)
    qr, tr = q[::-1], t[::-1]
    idx = np.arange(n + 1, dtype=np.int32)
    D = np.empty((m + 1, n + 1), dtype=np.int32)
    D[0] = idx
    for i in range(m):
        cur = np.empty(n + 1, dtype=np.int32)
        cur[0] = i + 1
        np.minimum(D[i, :-1] + (tr != qr[i]), D[i, 1:] + 1, out=cur[1:])
        D[i + 1] = np.minimum.accumulate(cur - idx) + idx
    return D[::-1, ::-1]


def walk(q, t):
    """the runs of the symbols q (other bytes 4) against t (other bytes 5), and E[0][0]"""
    m, n = len(q), len(t)
    E = _suffix_table(q, t)
    runs, i, j = [], 0, 0
    while i < m or j < n:
        e = int(E[i, j])
        if i < m and j < n and q[i] == t[j]:
            op, i, j = OP_EQ, i + 1, j + 1
        elif i < m and j < n and int(E[i + 1, j + 1]) + 1 == e:
            op, i, j = OP_X, i + 1, j + 1
        elif i < m and int(E[i + 1, j]) + 1 == e:
            op, i = OP_I, i + 1
        else:
            assert j < n and int(E[i, j + 1]) + 1 == e
            op, j = OP_D, j + 1
        if runs and runs[-1][1] == op:
            runs[-1][0] += 1
        else:
            runs.append([1, op])
    return [(k << 4) | op for k, op in runs], int(E[0, 0])


def align(read, strand, win, max_dist=None):
    """(d, a, b, runs) of the read against the window's bytes; None where edit_ref.infix gives None (not aligned: no runs)"""
    got = edit_ref.infix(read, strand, win, max_dist)
    if got is None:
        return None
    d, a, b = got
    q, t = edit_ref._syms(edit_ref.oriented(read, strand), 4), edit_ref._syms(edit_ref._bytes(win)[a:b], 5)
    runs, e00 = walk(q, t)
    assert e00 == d
    return d, a, b, runs


def cigar(runs):
    return "".join(f"{int(w) >> 4}{LETTER[int(w) & 15]}" for w in runs)


def check_invariants(read, strand, win, answer):
    """what follows from the definition, without the table: the counts, the run bound, the ends, and that every = base matches and no X base does"""
    d, a, b, runs = answer
    q, t = edit_ref._syms(edit_ref.oriented(read, strand), 4), edit_ref._syms(edit_ref._bytes(win)[a:b], 5)
    m, n = len(q), len(t)
    count = {OP_I: 0, OP_D: 0, OP_EQ: 0, OP_X: 0}
    i = j = 0
    for k, w in enumerate(runs):
        ln, op = int(w) >> 4, int(w) & 15
        assert op in count and ln > 0, (k, w)
        assert k == 0 or (int(runs[k - 1]) & 15) != op, "neighbouring runs are merged"
        count[op] += ln
        if op in (OP_EQ, OP_X):
            assert i + ln <= m and j + ln <= n
            same = q[i:i + ln] == t[j:j + ln]
            assert same.all() if op == OP_EQ else not same.any(), (k, w)
            i, j = i + ln, j + ln
        elif op == OP_I:
            i += ln
        else:
            j += ln
    assert (i, j) == (m, n)
    assert count[OP_X] + count[OP_I] + count[OP_D] == d
    assert count[OP_EQ] + count[OP_X] + count[OP_I] == m and count[OP_EQ] + count[OP_X] + count[OP_D] == n
    assert len(runs) <= 2 * d + 1
    assert not runs or ((int(runs[0]) & 15) != OP_D and (int(runs[-1]) & 15) != OP_D)
    assert m > 0 or not runs
