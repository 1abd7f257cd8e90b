"""Plain gzip streams for the gzip decoder tests (zlib, gzip, struct and random only): every DEFLATE form zlib writes on FASTA/FASTQ text and
on binary data, gzip framing (header fields, empty and concatenated members, trailing garbage) and corrupt streams.

good_cases() -> [(name, gzip bytes, inflated bytes)]; corrupt_cases() -> [(name, gzip bytes, (lo, hi))]: the decoder must fail with a
compressed byte offset in [lo, hi]."""
from __future__ import annotations

import random
import struct
import zlib

import bgzf_corpus as bc


def fasta_text(rng: random.Random, n: int) -> bytes:
    out, size = [], 0
    while size < n:
        L = rng.randrange(200, 3000)
        s = "".join(rng.choice("ACGT") for _ in range(L))
        rec = f">contig{rng.randrange(10**6)} some description\n" + "\n".join(s[i:i + 80] for i in range(0, L, 80)) + "\n"
        out.append(rec); size += len(rec)
    return "".join(out).encode()


def fastq_text(rng: random.Random, n: int) -> bytes:
    t = bc.fastq_text(rng, n)
    return t[:t.rfind(b"\n@") + 1] if b"\n@" in t else t


def member(raw: bytes, data: bytes, flags: int = 0, extra: bytes = b"", name: bytes = b"", comment: bytes = b"", crc: int | None = None,
           isize: int | None = None) -> bytes:
    """a gzip member around a raw deflate stream, with the optional header fields RFC 1952 allows"""
    h = bytes([0x1F, 0x8B, 8, flags]) + b"\0\0\0\0" + b"\0\x03"
    if flags & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flags & 8:
        h += name + b"\0"
    if flags & 16:
        h += comment + b"\0"
    if flags & 2:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    c = zlib.crc32(data) & 0xFFFFFFFF if crc is None else crc
    return h + raw + struct.pack("<II", c, (len(data) if isize is None else isize) & 0xFFFFFFFF)


def stored_deflate(data: bytes, block: int = 40000) -> bytes:
    """a raw deflate stream of hand-built stored blocks of `block` bytes, the final one holding the last bytes (zlib's encoder instead ends
    with a small or empty block, so its members never end in a long stored block)"""
    out = b""
    for i in range(0, max(len(data), 1), block):
        piece = data[i:i + block]
        out += bytes([1 if i + block >= len(data) else 0]) + struct.pack("<HH", len(piece), len(piece) ^ 0xFFFF) + piece
    return out


def gz(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, flush_every: int = 0, flush=zlib.Z_SYNC_FLUSH, **kw) -> bytes:
    return member(bc.deflate(data, level, strategy, flush_every, flush), data, **kw)


def good_cases(seed: int = 5, size: int = 150_000):
    rng = random.Random(seed)
    fq, fa = fastq_text(rng, size), fasta_text(rng, size)
    rnd = rng.randbytes(size // 3)
    cases = []
    for lvl in (1, 6, 9):
        cases.append((f"fastq_l{lvl}", gz(fq, lvl), fq))
        cases.append((f"fasta_l{lvl}", gz(fa, lvl), fa))
    cases.append(("fastq_l0_stored", gz(fq, 0), fq))
    cases.append(("fastq_stored_final_40000", member(stored_deflate(fq), fq), fq))
    for name, strat in (("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
        cases.append((f"fastq_{name}", gz(fq, 6, strat), fq))
    cases.append(("fastq_sync_flush", gz(fq, 6, flush_every=7001), fq))
    cases.append(("fastq_full_flush", gz(fq, 6, flush_every=12345, flush=zlib.Z_FULL_FLUSH), fq))
    cases.append(("random_binary", gz(rnd, 6), rnd))
    cases.append(("random_binary_stored", gz(rnd, 0), rnd))
    cases.append(("repetitive", gz(b"ACGT" * 60000, 9), b"ACGT" * 60000))
    cases.append(("empty_member", gz(b""), b""))
    cases.append(("header_fields", gz(fq[:20000], 6, flags=2 | 4 | 8 | 16, extra=b"AB\x02\x00xy", name=b"reads.fq", comment=b"a comment"),
                  fq[:20000]))
    a, b = fq[:size // 2], fa[:size // 3]
    cases.append(("two_members", gz(a, 6) + gz(b, 1, flags=8, name=b"b.fa"), a + b))
    cases.append(("members_with_empty", gz(b"") + gz(a, 9) + gz(b"") + gz(b, 6), a + b))
    cases.append(("trailing_garbage", gz(a, 6) + b"this is not a gzip member\0\0\0" * 3, a))
    cases.append(("trailing_zeros", gz(a, 6) + bytes(1000), a))
    cases.append(("trailing_one_byte", gz(a, 6) + b"\x1f", a))
    return cases


def corrupt_cases(seed: int = 9, size: int = 120_000):
    rng = random.Random(seed)
    fq = fastq_text(rng, size)
    good = gz(fq, 6)
    n = len(good)
    cases = [
        ("truncated_deflate", good[:n // 2], (n // 2 - 64, n // 2)),
        ("truncated_trailer", good[:n - 3], (n - 3, n - 3)),
        ("truncated_header", good[:7], (0, 7)),
        ("bad_crc", member(bc.deflate(fq), fq, crc=zlib.crc32(fq) ^ 1), (n - 8, n - 8)),
        ("bad_isize", member(bc.deflate(fq), fq, isize=len(fq) + 1), (n - 4, n - 4)),
        ("bad_method", good[:2] + b"\x07" + good[3:], (0, 0)),
        ("reserved_flag", good[:3] + b"\x20" + good[4:], (0, 0)),
        ("bad_header_crc", gz(fq, 6, flags=2)[:10] + b"\0\0" + gz(fq, 6, flags=2)[12:], (0, 0)),
        ("bad_second_header", good + good[:2] + b"\x07" + good[3:], (n, n)),
        ("btype3", member(b"\x07" + bc.deflate(fq)[1:], fq), (10, 10)),
    ]
    for i in range(4):                                           # flipped bits in the deflate data: an error at or behind the flip
        f = rng.randrange(n // 4, n - 16)
        cases.append((f"flip_{i}", good[:f] + bytes([good[f] ^ (1 << rng.randrange(8))]) + good[f + 1:], (f - 8, n)))
    return cases
