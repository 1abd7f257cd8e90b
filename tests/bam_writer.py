"""A small BGZF/BAM writer for test fixtures (zlib and struct only), and what `samtools fastq -n` makes of the same records.

A record is (name, read, flag): `read` is the read as sequenced, in letters of NT16 ("=ACMGRSVTWYHKDBN"); a record with flag 0x10 is stored
reverse-complemented, as an aligner stores a read mapped to the reverse strand.  The uncompressed stream is cut into BGZF blocks of
`block_bytes` regardless of record boundaries, so records span blocks whenever block_bytes is smaller than they are."""
from __future__ import annotations

import struct
import zlib

NT16 = "=ACMGRSVTWYHKDBN"
_CODE = {c: i for i, c in enumerate(NT16)}
_COMP = [int(f"{i:04b}"[::-1], 2) for i in range(16)]          # the complement of a 4-bit code is its bit reversal
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def revcomp(read: str) -> str:
    return "".join(NT16[_COMP[_CODE[c]]] for c in reversed(read))


def pack(read: str) -> bytes:
    """4-bit codes, two per byte, the first in the high nibble"""
    codes = [_CODE[c] for c in read] + ([0] if len(read) % 2 else [])
    return bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))


def bgzf_block(data: bytes, level: int = 6) -> bytes:
    assert len(data) <= 65536
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    cdata = c.compress(data) + c.flush()
    bsize = 18 + len(cdata) + 8
    assert bsize <= 65536, "block does not compress into 64 KiB: use smaller block_bytes"
    hdr = b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
    return hdr + cdata + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


def record_bytes(name: str, read: str, flag: int, tags: bytes = b"") -> bytes:
    stored = revcomp(read) if flag & 0x10 else read
    nm = name.encode() + b"\0"
    body = struct.pack("<iiBBHHHi", -1, -1, len(nm), 255, 4680, 0, flag, len(read)) + struct.pack("<iii", -1, -1, 0)
    body += nm + pack(stored) + b"\xff" * len(read) + tags
    return struct.pack("<i", len(body)) + body


def header_bytes(refs=(("chr1", 1000),), text: str = "@HD\tVN:1.6\tSO:unknown\n") -> bytes:
    t = text.encode()
    h = b"BAM\1" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(refs))
    for n, L in refs:
        nb = n.encode() + b"\0"
        h += struct.pack("<i", len(nb)) + nb + struct.pack("<i", L)
    return h


def bam_stream(records) -> bytes:
    return header_bytes() + b"".join(record_bytes(n, r, f) for n, r, f in records)


def write_bgzf(path: str, data: bytes, block_bytes: int = 65280, eof: bool = True) -> None:
    with open(path, "wb") as f:
        for i in range(0, len(data), block_bytes):
            f.write(bgzf_block(data[i:i + block_bytes]))
        f.write(EOF_BLOCK if eof else b"")


def write_bam(path: str, records, block_bytes: int = 65280, eof: bool = True) -> None:
    write_bgzf(path, bam_stream(records), block_bytes, eof)


def kept(records):
    """the records samtools fastq writes (secondary 0x100 and supplementary 0x800 ones are not), as (name, read as sequenced)"""
    return [(n, r) for n, r, f in records if not f & 0x900]


def write_fastq(path: str, records) -> None:
    """`samtools fastq -n` of the same records (the mapper never reads qualities: a fixed letter stands in for them)"""
    with open(path, "w") as f:
        for n, r in kept(records):
            f.write(f"@{n}\n{r}\n+\n{'I' * len(r)}\n")
