"""Problems for the edit-distance tests (tests/test_edit_core.py on the host build): each one is
(read, strand, window, max_dist) with max_dist None for "no cap" — the read as stored, the window's bytes as they lie on the contig."""
import numpy as np

import edit_ref

ALPHA = np.frombuffer(b"ACGT", dtype=np.uint8)


def dna(rng, n):
    return ALPHA[rng.integers(0, 4, size=n)].tobytes()


def mutate(rng, s, rate):
    """substitutions, insertions and deletions at `rate` per base, a third each"""
    out = bytearray()
    for c in s:
        u = rng.random()
        if u < rate / 3:
            out.append(int(ALPHA[rng.integers(0, 4)]))
        elif u < 2 * rate / 3:
            out.append(c)
            out.append(int(ALPHA[rng.integers(0, 4)]))
        elif u >= rate:
            out.append(c)
    return bytes(out)


def sprinkle(rng, s, frac, what):
    """`what` bytes at a fraction of the positions (N, IUPAC), and some bases in lower case"""
    b = bytearray(s)
    for p in np.flatnonzero(rng.random(len(b)) < frac):
        b[p] = what[int(rng.integers(0, len(what)))]
    for p in np.flatnonzero(rng.random(len(b)) < frac):
        b[p] = ord(chr(b[p]).lower())
    return bytes(b)


def stored(read, strand):
    """the bytes a read set holds for a read that aligns as `read` on that strand"""
    return edit_ref.oriented(read, -1) if strand < 0 else read


def planted(rng, m, left, right, rate, strand=1, dirt=0.0):
    """a window of left + m + right bases and a read made from its middle with errors"""
    win = dna(rng, left + m + right)
    read = mutate(rng, win[left:left + m], rate)
    if dirt:
        win, read = sprinkle(rng, win, dirt, b"NRYK"), sprinkle(rng, read, dirt, b"NnMS")
    return stored(read, strand), strand, win


def random_problem(rng, k):
    m = int(rng.integers(0, 91))
    kind = k % 5
    if kind == 0:                                                   # unrelated strings, no cap
        return dna(rng, m), int(rng.choice([-1, 1])), dna(rng, int(rng.integers(0, 140))), None
    left, right = (int(x) for x in rng.integers(0, 40, size=2))
    read, strand, win = planted(rng, m, left, right, float(rng.choice([0.0, 0.05, 0.15, 0.3])), int(rng.choice([-1, 1])), 0.04 if kind == 1 else 0.0)
    if kind == 2:                                                   # a truncated window: the read hangs over one end
        cut = int(rng.integers(0, len(win) + 1))
        win = win[cut:] if rng.random() < 0.5 else win[:cut]
    md = None if kind == 3 else edit_ref.cap(len(read), float(rng.choice([80.0, 90.0, 70.0])))
    return read, strand, win, md


def at_cap_pair(rng):
    """two problems with substitutions only, far enough apart that d is their number: d == max_dist (aligned) and d == max_dist + 1 (not)"""
    m = 60
    win = dna(rng, 20 + m + 20)
    read = bytearray(win[20:20 + m])
    for p in (5, 17, 29, 41, 53):
        read[p] = ord("ACGT"[("ACGT".index(chr(read[p])) + 1) % 4])
    return (bytes(read), 1, win, 5), (bytes(read), 1, win, 4)


def edge_problems(rng):
    out = []
    for m in (0, 1, 15, 16, 17, 63, 64, 65):
        for strand in (1, -1):
            out.append(planted(rng, m, 9, 11, 0.1, strand) + (None,))
            out.append(planted(rng, m, 0, 0, 0.0, strand) + (edit_ref.cap(m),))
    out.append((dna(rng, 20), 1, b"", None))                        # an empty window: every base is an insertion
    out.append((dna(rng, 20), 1, b"", 6))
    out.append((b"", 1, b"", None))
    r, s, w = planted(rng, 50, 0, 0, 0.05)
    out += [(r, s, w[:30], None), (r, -1, w[10:35], None), (r, s, w[:30], 12)]     # a window shorter than the read
    out += list(at_cap_pair(rng))
    for strand in (1, -1):
        out.append(planted(rng, 70, 13, 5, 0.08, strand, dirt=0.1) + (None,))      # N, IUPAC and lower case on both sides
    out.append((b"ACGTNNNNACGTacgt", 1, b"TTACGTNNNNACGTACGTTT", None))            # an N matches nothing, not even an N
    out.append((b"NNNN", -1, b"NNNNNN", None))
    out.append((b"acgtRYacgt", -1, b"ggacgtrYacgtgg", None))
    return out
