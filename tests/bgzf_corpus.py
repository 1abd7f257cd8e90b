"""BGZF blocks for the inflate tests (zlib, struct and random only): good blocks covering every DEFLATE form zlib writes, hand-built streams
for what zlib never writes (distance 32 768, block type 3), and corrupt blocks with the status the decoder must give each.

A case is (name, block bytes, expected inflated bytes or None, expected status).  Statuses: 0 ok, 1 deflate stream invalid, 2 length !=
ISIZE, 3 CRC32 mismatch, 4 malformed header."""
from __future__ import annotations

import random
import struct
import zlib

import bam_writer as bw

OK, BAD_STREAM, BAD_LENGTH, BAD_CRC, BAD_HEADER = 0, 1, 2, 3, 4


def member(cdata: bytes, data: bytes, crc: int | None = None, isize: int | None = None) -> bytes:
    """a BGZF block around a raw deflate stream (no size limit: the decoder does not need one)"""
    bsize = 18 + len(cdata) + 8
    hdr = b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, (bsize - 1) & 0xFFFF)
    c = zlib.crc32(data) & 0xFFFFFFFF if crc is None else crc
    return hdr + cdata + struct.pack("<II", c, len(data) if isize is None else isize)


def deflate(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, flush_every: int = 0, flush=zlib.Z_SYNC_FLUSH) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    out = b""
    for i in range(0, len(data), flush_every):
        out += c.compress(data[i:i + flush_every]) + c.flush(flush)
    return out + c.flush()


class BitWriter:
    """LSB-first bit stream; Huffman codes go in MSB first"""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, v: int, n: int):
        self.v |= (v & ((1 << n) - 1)) << self.n
        self.n += n

    def code(self, c: int, n: int):
        self.put(int(f"{c:0{n}b}"[::-1], 2), n)

    def bytes(self) -> bytes:
        return self.v.to_bytes((self.n + 7) // 8, "little")


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def fixed_sym(w: BitWriter, s: int):
    if s < 144: w.code(0x30 + s, 8)
    elif s < 256: w.code(0x190 + s - 144, 9)
    elif s < 280: w.code(s - 256, 7)
    else: w.code(0xC0 + s - 280, 8)


def fixed_stream(items, final: bool = True, w: BitWriter | None = None, btype: int = 1) -> BitWriter:
    """one fixed-Huffman block of items: an int is a literal byte, a (length, distance) pair a match; ('dsym', n) a raw distance symbol"""
    w = w or BitWriter()
    w.put(1 if final else 0, 1)
    w.put(btype, 2)
    for it in items:
        if isinstance(it, int):
            fixed_sym(w, it)
            continue
        L, D = it
        i = max(k for k in range(29) if LBASE[k] <= L)
        fixed_sym(w, 257 + i); w.put(L - LBASE[i], LEXT[i])
        j = max(k for k in range(30) if DBASE[k] <= D)
        w.code(j, 5); w.put(D - DBASE[j], DEXT[j])
    fixed_sym(w, 256)
    return w


def fastq_text(rng: random.Random, n: int) -> bytes:
    out = []
    while sum(map(len, out)) < n:
        L = rng.randrange(50, 400)
        s = "".join(rng.choice("ACGT") for _ in range(L))
        out.append(f"@read{rng.randrange(10**6)} len={L}\n{s}\n+\n{''.join(rng.choice('#+5?AEIJ') for _ in range(L))}\n")
    return "".join(out).encode()[:n]


def bam_like(rng: random.Random, n: int) -> bytes:
    recs = [(f"r{i}", "".join(rng.choice("ACGTN") for _ in range(rng.randrange(20, 500))), rng.choice([0, 0x10])) for i in range(n // 200 + 2)]
    return bw.bam_stream(recs)[:n]


def good_cases(seed: int = 7):
    rng = random.Random(seed)
    fq, bam, rnd = fastq_text(rng, 60000), bam_like(rng, 60000), rng.randbytes(40000)
    cases = []
    for lvl in (0, 1, 6, 9):
        for nm, d in (("fastq", fq), ("bam", bam), ("random", rnd)):
            cases.append((f"level{lvl}_{nm}", d, deflate(d, lvl)))
    for st, nm in ((zlib.Z_FILTERED, "filtered"), (zlib.Z_HUFFMAN_ONLY, "huffman_only"), (zlib.Z_RLE, "rle"), (zlib.Z_FIXED, "fixed")):
        cases.append((f"strategy_{nm}_fastq", fq, deflate(fq, 6, st)))
        cases.append((f"strategy_{nm}_bam", bam, deflate(bam, 6, st)))
    cases.append(("sync_flush", fq, deflate(fq, 6, flush_every=7000, flush=zlib.Z_SYNC_FLUSH)))
    cases.append(("full_flush", bam, deflate(bam, 6, flush_every=5000, flush=zlib.Z_FULL_FLUSH)))
    cases.append(("sync_flush_tiny", fq[:3000], deflate(fq[:3000], 9, flush_every=100)))
    big = fastq_text(rng, 65536)
    cases.append(("block_65536", big, deflate(big, 6)))
    cases.append(("block_65536_stored", rnd[:30000] + rnd[:30000] + rnd[:5536], deflate(rnd[:30000] + rnd[:30000] + rnd[:5536], 0)))
    cases.append(("run_one_byte", b"A" * 65536, deflate(b"A" * 65536, 9)))
    cases.append(("run_short", b"AC" * 700 + b"G", deflate(b"AC" * 700 + b"G", 9)))
    cases.append(("empty", b"", deflate(b"", 6)))
    cases.append(("one_byte", b"x", deflate(b"x", 6)))
    # distance 32 768 (zlib's deflate never goes further than 32 506): literals, then matches reaching back exactly 32 768 bytes
    lits = list(rng.randbytes(32768))
    far = fixed_stream(lits + [(258, 32768), (100, 32768), (3, 32768)])
    cases.append(("distance_32768", bytes(lits) + bytes(lits[:258]) + bytes(lits[258:358]) + bytes(lits[358:361]), far.bytes()))
    # overlapping matches of every short period
    items, data = [], b""
    for d in range(1, 80):
        pat = rng.randbytes(d)
        items += list(pat) + [(rng.randrange(3, 259), d)]
        L = items[-1][0]
        data += pat + (pat * (L // d + 2))[:L]
    cases.append(("overlap_periods", data, fixed_stream(items).bytes()))
    # several fixed blocks in a row, then an empty stored block as the final one
    w = fixed_stream(list(b"hello "), final=False)
    w = fixed_stream(list(b"world ") + [(5, 6)], final=False, w=w)
    w.put(1, 1); w.put(0, 2); w.put(0, (-w.n) % 8); w.put(0, 16); w.put(0xFFFF, 16)
    cases.append(("fixed_then_empty_stored", b"hello world world", w.bytes()))
    out = [(nm, member(c, d), d, OK) for nm, d, c in cases]
    out.append(("eof_block", bw.EOF_BLOCK, b"", OK))
    return out


def corrupt_cases(seed: int = 11):
    rng = random.Random(seed)
    d = fastq_text(rng, 20000)
    c = deflate(d, 6)
    crc = zlib.crc32(d) & 0xFFFFFFFF
    out = [
        ("flipped_crc", member(c, d, crc=crc ^ 0x10), BAD_CRC),
        ("isize_larger", member(c, d, isize=len(d) + 1), BAD_LENGTH),
        ("isize_smaller", member(c, d, isize=len(d) - 1), BAD_STREAM),
        ("isize_over_64k", member(c, d, isize=65537), BAD_LENGTH),
        ("truncated_stream", member(c[:len(c) // 2], d), BAD_STREAM),
        ("truncated_last_byte", member(c[:-1], d), BAD_STREAM),
        ("short_header", bw.EOF_BLOCK[:25], BAD_HEADER),
        ("xlen_overrun", bw.EOF_BLOCK[:10] + struct.pack("<H", 200) + bw.EOF_BLOCK[12:], BAD_HEADER),
    ]
    w = BitWriter(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(15, 4)
    for _ in range(19): w.put(1, 3)                              # 19 code-length codes of length 1: over-subscribed
    out.append(("oversubscribed_code_lengths", member(w.bytes() + b"\0" * 8, b"x"), BAD_STREAM))
    w = BitWriter(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(0, 4)
    w.put(1, 3); w.put(0, 3); w.put(0, 3); w.put(0, 3)           # one code-length code of length 1: incomplete
    out.append(("incomplete_code_lengths", member(w.bytes() + b"\0" * 8, b"x"), BAD_STREAM))
    out.append(("distance_before_start", member(fixed_stream(list(b"abc") + [(3, 4)]).bytes(), b"abcabc"), BAD_STREAM))
    out.append(("distance_symbol_30", member(fixed_stream([]).bytes()[:0] + _dist_sym_stream(30), b"aaaa"), BAD_STREAM))
    out.append(("block_type_3", member(fixed_stream(list(b"abc"), btype=3).bytes(), b"abc"), BAD_STREAM))
    bad_stored = BitWriter(); bad_stored.put(1, 1); bad_stored.put(0, 2); bad_stored.put(0, 5); bad_stored.put(5, 16); bad_stored.put(5, 16)
    out.append(("stored_nlen_mismatch", member(bad_stored.bytes() + b"hello", b"hello"), BAD_STREAM))
    out.append(("garbage", member(rng.randbytes(300), b"y" * 1000), None))
    return out


def _dist_sym_stream(sym: int) -> bytes:
    w = BitWriter(); w.put(1, 1); w.put(1, 2)
    fixed_sym(w, ord("a"))
    fixed_sym(w, 257)                                             # length 3
    w.code(sym, 5)
    fixed_sym(w, 256)
    return w.bytes()


def pack(blocks) -> bytes:
    return b"".join(struct.pack("<I", len(b)) + b for b in blocks)
