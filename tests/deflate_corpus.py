"""Inputs and checks shared by the BGZF deflate tests (CPU: tests/test_deflate_core.py, GPU: tests/test_gpu_deflate.py): the corpus, the
synthetic mapping text the ratio condition is stated on, and what every written member must satisfy.  zlib, gzip, struct and random only."""
from __future__ import annotations

import gzip
import random
import struct
import zlib

import bgzf_corpus as bc

BLOCK_IN = 0xff00
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
RATIO_BOUND = 1.15                                               # against zlib level 1 on the same blocks


def mapping_text(n_bytes: int, seed: int = 3) -> bytes:
    """lines in the shape of the mappings file: 14 fields separated by spaces, UUID-style read names (several lines per read), 3 000 contig
    names, random coordinates, an identity and trailing counts"""
    rng = random.Random(seed)
    contigs = [f"kraken:taxid|{rng.randrange(100, 2000000)}|NZ_{rng.choice('ABCJLP')}{rng.choice('ABCDEFGHJKLMNPQRSTUVWXYZ')}{rng.randrange(10**6, 10**7)}.{rng.randrange(1, 4)}"
               for _ in range(3000)]
    out, size = [], 0
    while size < n_bytes:
        name = "%08x-%04x-%04x-%04x-%012x" % (rng.getrandbits(32), rng.getrandbits(16), rng.getrandbits(16), rng.getrandbits(16), rng.getrandbits(48))
        rlen = rng.randrange(1000, 30000)
        near = rng.sample(contigs, 3)
        for _ in range(rng.choice((1, 1, 2, 3, 4, 6, 9))):
            qs = rng.randrange(0, 50)
            qe = rlen - rng.randrange(0, 50)
            rs = rng.randrange(0, 5_000_000)
            sk = rng.randrange(40, 600)
            line = (f"{name} {qs} {qe} {rlen} {rng.choice('+-')} {rng.choice(near)} {rs} {rs + qe - qs + rng.randrange(-200, 200)} "
                    f"{rng.randrange(10, sk)} {sk} {rng.uniform(80, 100):.4f} {rng.randrange(1, 500)} {rng.uniform(0, 1):.6f} {rng.randrange(0, 60)}\n")
            out.append(line); size += len(line)
    return "".join(out).encode()[:n_bytes]


def corpus(seed: int = 5):
    """(name, bytes): sizes around the block size, the degenerate code tables, the window edge, compressible and incompressible data"""
    rng = random.Random(seed)
    p32768, p32769 = rng.randbytes(32768), rng.randbytes(32769)
    mt = mapping_text(3 * BLOCK_IN + 1234)
    return [
        ("one_byte", b"x"),
        ("two_distinct", b"ab"),
        ("size_65279", bc.fastq_text(rng, 65279)),
        ("size_65280", bc.fastq_text(rng, 65280)),
        ("size_65281", bc.fastq_text(rng, 65281)),
        ("one_repeated_byte", b"A" * 70000),                     # distance codes: a single one in use
        ("single_value_short", b"z" * 40),                       # no match (the first step finds none): no distance code at all
        ("all_256_values", bytes(range(256)) * 64 + bytes(rng.randrange(256) for _ in range(5000)) + bytes(range(256)) * 8),
        ("period_32768", p32768 + p32768[:32512]),
        ("period_32769", p32769 + p32769[:32511]),
        ("random", rng.randbytes(200000)),
        ("fastq", bc.fastq_text(rng, 150000)),
        ("bam_like", bc.bam_like(rng, 150000)),
        ("mapping_text", mt),
        ("skewed_lengths", b"".join(bytes([i]) * (1 << min(i, 14)) for i in range(24))[:65280]),   # frequencies 1, 2, 4, ...: the length limit
    ]


def marker_pair(seed: int = 21):
    """300 random bytes, a run of one byte, the 300 bytes again: 32 768 bytes after their first occurrence, and 32 769"""
    m = random.Random(seed).randbytes(300)
    return m + b"A" * (32768 - 300) + m, m + b"A" * (32769 - 300) + m


def members(comp: bytes):
    """the BGZF members of comp (each checked: magic, BC subfield, BSIZE = member length - 1)"""
    out, at = [], 0
    while at < len(comp):
        assert comp[at:at + 4] == b"\x1f\x8b\x08\x04" and comp[at + 10:at + 16] == b"\x06\x00BC\x02\x00", at
        bsize = struct.unpack_from("<H", comp, at + 16)[0] + 1
        assert 26 <= bsize <= 65536 and at + bsize <= len(comp), (at, bsize)
        out.append(comp[at:at + bsize]); at += bsize
    return out


def is_stored(member: bytes) -> bool:
    return (member[18] >> 1) & 3 == 0


def check_container(comp: bytes, data: bytes):
    """every member is BGZF with ISIZE <= 65 280, inflates with zlib to its slice of data with the right CRC and nothing behind it; the
    members cut the input at 65 280 bytes; Python's gzip reads the whole file with the EOF block behind it"""
    ms = members(comp)
    assert len(ms) == (len(data) + BLOCK_IN - 1) // BLOCK_IN
    at = 0
    for m in ms:
        crc, isize = struct.unpack("<II", m[-8:])
        assert isize == min(BLOCK_IN, len(data) - at), (at, isize)
        d = zlib.decompressobj(31)
        got = d.decompress(m)
        assert d.eof and d.unused_data == b"" and got == data[at:at + isize], at
        assert crc == zlib.crc32(got) & 0xFFFFFFFF
        at += isize
    assert at == len(data)
    assert gzip.decompress(comp + EOF_BLOCK) == data
    return ms


def zlib1_size(data: bytes) -> int:
    """what bgzip -l 1 writes for data: zlib level 1 raw deflate of each 65 280-byte block + 26 bytes"""
    return sum(len(bc.deflate(data[i:i + BLOCK_IN], 1)) + 26 for i in range(0, len(data), BLOCK_IN))
