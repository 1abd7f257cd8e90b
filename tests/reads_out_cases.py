"""The sets and selections that hold mm_reads_out_core.hpp (tests/test_reads_out_core.py, CPU) and mm_reads_encode (tests/test_gpu_reads_out.py) to
tests/reads_out_ref.py.  A read is (bases as given, Phred values or None)."""
import random

LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4099]
IUPAC = "RYSWKMBDHVN"


def _acgt(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _with_run(rng, n, at, length, letter):
    s = _acgt(rng, n)
    return s[:at] + letter * length + s[at + length:]


def edge_reads(seed=11):
    """every length of LENGTHS; exception runs of 1 and 40 bytes that start and end on the 16- and 32-base word edges and at the first and last base; lower
    case; IUPAC letters; quality bytes 0 and 93; reads with and without qualities"""
    rng = random.Random(seed)
    reads = [_acgt(rng, n) for n in LENGTHS]
    n = 200
    for length in (1, 40):
        for edge in (16, 32, 64, 96):
            reads.append(_with_run(rng, n, edge, length, "N"))              # starts on the edge
            reads.append(_with_run(rng, n, edge - length, length, "R"))     # ends on it
            reads.append(_with_run(rng, n, edge - 1, length, "Y"))          # straddles it
        reads.append(_with_run(rng, n, 0, length, "N"))                     # the read's first base
        reads.append(_with_run(rng, n, n - length, length, "W"))            # its last
    reads.append("N")
    reads.append("N" * 40)
    reads.append(_acgt(rng, 77).lower())
    reads.append("".join(rng.choice("acgtnACGTN") for _ in range(130)))
    reads.append("".join(rng.choice(IUPAC) for _ in range(90)))
    reads.append("".join(rng.choice("ACGT" * 5 + IUPAC) for _ in range(4099)))   # runs all over a long read
    quals = []
    for i, r in enumerate(reads):
        if i % 3 == 2:
            quals.append(None)
        else:
            q = [rng.randrange(0, 94) for _ in r]
            if q:
                q[0] = 0; q[-1] = 93
            quals.append(q)
    return [r.encode() for r in reads], quals


def names_for(n, seed=5):
    """printable names of 1 to 254 bytes: the first of 1 byte, the second of 254"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        L = 1 if i == 0 else 254 if i == 1 else rng.randrange(1, 40)
        out.append(bytes(rng.randrange(0x21, 0x7F) for _ in range(L)))
    return out


def selections(n, seed=3):
    rng = random.Random(seed)
    return {"none": [], "all": list(range(n)), "every_third": list(range(0, n, 3)), "permuted_with_repeats": [rng.randrange(n) for _ in range(n + n // 2)]}


def random_sets(count=200, seed=9):
    """small random sets: (reads, quals, selection, names)"""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        n = rng.randrange(1, 6)
        reads, quals = [], []
        for _ in range(n):
            L = rng.choice([0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 70])
            reads.append("".join(rng.choice("ACGTacgt" * 3 + IUPAC) for _ in range(L)).encode())
            quals.append(None if rng.random() < 0.3 else [rng.choice([0, 93, 0xFF, rng.randrange(94)]) for _ in range(L)])
        sel = [rng.randrange(n) for _ in range(rng.randrange(0, 8))]
        names = [bytes(rng.randrange(0x21, 0x7F) for _ in range(rng.choice([1, 2, 3, 4, 5, 30, 254]))) for _ in sel]
        out.append((reads, quals, sel, names))
    return out


def bad_records():
    """(rule, read index, name) against a set of 3 reads"""
    return [(1, 3, b"r"), (1, -1, b"r"), (1, 1 << 30, b"r"), (2, 0, b""), (2, 0, b"x" * 255), (3, 0, b"a b"), (3, 0, b"a\x7f"), (3, 0, b"\x20"), (3, 0, b"ab\n"), (3, 0, b"\xc3\xa4"),
            (1, 3, b""), (2, 0, b" " * 255)]
