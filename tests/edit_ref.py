"""The naive restatement of the exact edit distances of mappings (metamaps_amd/csrc/mm_edit_core.hpp has the definition): a plain
dynamic programme, one numpy row per read base.  The infix DP (first row 0: the window's start is free) gives d and the smallest end b; the anchored
DP of the reversed strings (first row 0, 1, 2, ...) gives the largest start a.  Also the window and cap rules."""
import math

import numpy as np

MAX_READ = 65536
_COMP = {ord("A"): "T", ord("C"): "G", ord("G"): "C", ord("T"): "A"}


def pad(L):
    return 64 + L // 16


def window(ref_start, L, C):
    ws = min(max(0, ref_start - pad(L)), C)
    we = max(min(C, ref_start + L + pad(L)), ws)
    return ws, we


def cap(L, pi=80.0):
    return max(0, int(math.floor(1.5 * float(L) * (100.0 - float(np.float32(pi))) / 100.0)))


def _bytes(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def oriented(read, strand):
    """the read as it is aligned: upper-cased; for strand -1 the reverse complement (a byte that is not A C G T stays one that matches nothing)"""
    r = _bytes(read).upper()
    if strand > 0:
        return r
    return "".join(_COMP.get(c, "N") for c in reversed(r)).encode()


def _syms(s, other):
    """A C G T -> 0 .. 3; everything else -> `other`"""
    t = np.full(256, other, dtype=np.int16)
    for k, c in enumerate(b"ACGT"):
        t[c] = k
        t[c + 32] = k
    return t[np.frombuffer(_bytes(s), dtype=np.uint8)]


def _last_row(q, r, anchored):
    """the last row of the DP of q (rows) against r (columns)"""
    n = len(r)
    idx = np.arange(n + 1, dtype=np.int64)
    prev = idx.copy() if anchored else np.zeros(n + 1, dtype=np.int64)
    for i in range(len(q)):
        cur = np.empty(n + 1, dtype=np.int64)
        cur[0] = i + 1
        np.minimum(prev[:-1] + (r != q[i]), prev[1:] + 1, out=cur[1:])
        prev = np.minimum.accumulate(cur - idx) + idx              # (the horizontal dependency: cur[j] = min over j' <= j of cur[j'] + j - j')
    return prev


def infix(read, strand, win, max_dist=None):
    """(d, a, b) of the read against the window's bytes, a and b in window coordinates (half-open); None if d > max_dist or the read is too long"""
    if len(read) > MAX_READ:
        return None
    q, r = _syms(oriented(read, strand), 4), _syms(win, 5)
    row = _last_row(q, r, False)
    d = int(row.min())
    if max_dist is not None and d > max_dist:
        return None
    b = int(np.argmax(row == d))
    back = _last_row(q[::-1], r[:b][::-1], True)
    assert int(back.min()) == d
    return d, b - int(np.argmax(back == d)), b


def record(read, strand, contig, ref_start, pi=80.0):
    """a mapping record by the window and cap rules: (d, first, last) in 0-based inclusive contig coordinates, or None (not aligned)"""
    ws, we = window(ref_start, len(read), len(contig))
    got = infix(read, strand, _bytes(contig)[ws:we], cap(len(read), pi))
    return None if got is None else (got[0], ws + got[1], ws + got[2] - 1)
