"""CPU test of the CLI's BAM reader (metamaps_amd/csrc/host/bam_reader.hpp, built with g++ from tests/test_bam_reader.cpp) against the BAM
writer of tests/bam_writer.py: names, lengths, 4-bit code bytes and flags come out as written, secondary and supplementary records are
skipped, records that span BGZF blocks (and inflate segments) come out whole, parallel and sequential inflate agree, BAM is told from
FASTA/FASTQ(.gz) by content, and every malformed input gets its error."""
import gzip
import os
import random
import struct
import subprocess

import pytest

import bam_writer as bw

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("br") / "t")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-o", e, os.path.join(HERE, "test_bam_reader.cpp"), "-lz"], check=True, timeout=300)
    return e


def _records(rng, n, long_read=False):
    recs = []
    for i in range(n):
        L = rng.choice([0, 1, 15, 16, 17, 31, 33, 150, 1000, 5000]) if i % 3 else rng.randrange(0, 300)
        alpha = bw.NT16 if i % 4 == 0 else "ACGT" * 6 + "N"
        read = "".join(rng.choice(alpha) for _ in range(L))
        flag = rng.choice([0, 0, 0x10, 0x10, 0x100, 0x800, 0x110, 0x4, 0x1 | 0x40, 0x1 | 0x80 | 0x10])
        recs.append((f"read{i}:{rng.randrange(10**6)}", read, flag))
    if long_read:
        L = (4 << 20) + 4099                                       # crosses the host packer's 4-Mbase piece boundary
        recs.append(("long_fwd", "".join(rng.choice("ACGT") for _ in range(L - 40)) + "N" * 40, 0))
        recs.append(("long_rev", "ACGTN" * (L // 5), 0x10))
    return recs


def _run(exe, path, threads=1, all_=False, max_len=None):
    args = [exe, "read", path, str(threads)] + (["all" if all_ else "kept"]) + ([str(max_len)] if max_len is not None else [])
    return subprocess.run(args, capture_output=True, timeout=600, text=True)


def _parse(out):
    lines = out.strip("\n").split("\n")
    recs = [tuple(l.split("\t")) for l in lines[:-1]]
    return recs, lines[-1]


def _expect(recs, all_=False):
    out = []
    for n, r, f in recs:
        if not all_ and f & 0x900:
            continue
        stored = bw.revcomp(r) if f & 0x10 else r
        out.append((n, str(len(r)), str(f), bw.pack(stored).hex(), r))
    return out


@pytest.mark.parametrize("block_bytes", [65280, 4000, 333])
def test_records_as_written(exe, tmp_path, block_bytes):
    rng = random.Random(block_bytes)
    recs = _records(rng, 400)
    p = str(tmp_path / "r.bam")
    bw.write_bam(p, recs, block_bytes=block_bytes)
    r = _run(exe, p)
    assert r.returncode == 0, r.stdout + r.stderr
    got, tail = _parse(r.stdout)
    assert got == _expect(recs)
    assert tail.endswith("eof 1") and "EOF marker" not in r.stderr
    r = _run(exe, p, all_=True)                                    # nothing but the 0x900 records was left out
    assert _parse(r.stdout)[0] == _expect(recs, all_=True)


def test_every_code_and_its_complement(exe, tmp_path):
    recs = [("fwd", bw.NT16 * 3, 0), ("rev", bw.NT16 * 3, 0x10), ("odd", bw.NT16[:15], 0x10)]
    p = str(tmp_path / "c.bam")
    bw.write_bam(p, recs)
    got, _ = _parse(_run(exe, p).stdout)
    assert [g[4] for g in got] == [r for _, r, _ in recs]
    assert got[1][3] == bw.pack("NVHMDRWABSYCKGT=" * 3).hex()      # samtools' complement table: A<->T, C<->G, M<->K, R<->Y, V<->B, H<->D


def test_parallel_inflate_and_segments(exe, tmp_path):
    rng = random.Random(7)
    recs = _records(rng, 3000, long_read=True)
    p = str(tmp_path / "big.bam")
    bw.write_bam(p, recs, block_bytes=1500)                        # > 1024 blocks: several inflate segments, records across them
    one, eight = _run(exe, p, threads=1), _run(exe, p, threads=8)
    assert one.returncode == 0 and eight.returncode == 0, one.stdout[-500:] + one.stderr
    assert one.stdout == eight.stdout
    got, tail = _parse(eight.stdout)
    assert got == _expect(recs)
    assert int(tail.split()[1]) > 2 * 1024


def test_detect_by_content(exe, tmp_path):
    rng = random.Random(3)
    recs = _records(rng, 20)
    bam = str(tmp_path / "reads.fq")                               # a BAM under a FASTQ name
    bw.write_bam(bam, recs)
    fq = str(tmp_path / "reads.bam")                               # and a FASTQ under a BAM name
    bw.write_fastq(fq, recs)
    with open(fq, "rb") as f, gzip.open(str(tmp_path / "r.fq.gz"), "wb") as g:
        g.write(f.read())
    bgz = str(tmp_path / "bgzf.fq.gz")                             # BGZF, but not BAM inside (bgzip of a FASTQ)
    bw.write_bgzf(bgz, open(fq, "rb").read())
    empty = str(tmp_path / "empty")
    open(empty, "wb").close()
    r = subprocess.run([exe, "detect", bam, fq, str(tmp_path / "r.fq.gz"), bgz, empty, str(tmp_path / "missing")], capture_output=True, text=True, timeout=60)
    assert r.stdout.split() == ["1", "0", "0", "0", "0", "0"]


def test_missing_eof_marker_warns(exe, tmp_path):
    rng = random.Random(5)
    recs = _records(rng, 50)
    p = str(tmp_path / "noeof.bam")
    bw.write_bam(p, recs, block_bytes=2000, eof=False)
    r = _run(exe, p)
    assert r.returncode == 0
    got, tail = _parse(r.stdout)
    assert got == _expect(recs) and tail.endswith("eof 0")
    assert "EOF marker is absent" in r.stderr


def _bad(exe, tmp_path, data, **kw):
    p = str(tmp_path / "bad.bam")
    open(p, "wb").write(data)
    r = _run(exe, p, **kw)
    assert r.returncode == 2, r.stdout + r.stderr
    return r.stdout


def test_malformed_inputs(exe, tmp_path):
    rng = random.Random(11)
    recs = _records(rng, 60)
    stream = bw.bam_stream(recs)
    good = b"".join(bw.bgzf_block(stream[i:i + 3000]) for i in range(0, len(stream), 3000))
    # a truncated BGZF block: the file ends inside one
    assert "truncated BGZF block" in _bad(exe, tmp_path, good[:len(good) - 700])
    # a truncated record: the stream ends inside a record, all blocks whole
    cut = len(bw.header_bytes()) + len(bw.record_bytes(*recs[0])) + 10
    assert "truncated BAM record" in _bad(exe, tmp_path, bw.bgzf_block(stream[:cut]) + bw.EOF_BLOCK)
    # bad magic: not BAM inside the BGZF, and not BGZF at all
    assert "bad magic" in _bad(exe, tmp_path, bw.bgzf_block(b"BAM\2" + stream[4:3000]) + bw.EOF_BLOCK)
    assert "bad magic" in _bad(exe, tmp_path, b"@r1\nACGT\n+\nIIII\n" * 10)
    first = bw.bgzf_block(stream[:3000])
    assert "bad magic" in _bad(exe, tmp_path, first + b"\0" * 100)   # a block boundary where no BGZF block starts
    # a corrupted block (CRC)
    blk = bytearray(bw.bgzf_block(stream[:3000]))
    blk[-6] ^= 0xff
    assert "CRC" in _bad(exe, tmp_path, bytes(blk) + bw.EOF_BLOCK)
    # l_seq above the limit (the limit is an argument of the reader: the CLI gives the library's 2^29 - 1)
    big = bw.header_bytes() + bw.record_bytes("r", "ACGT" * 300, 0)
    assert "longer than the limit" in _bad(exe, tmp_path, bw.bgzf_block(big) + bw.EOF_BLOCK, max_len=1000)
    huge = bytearray(bw.header_bytes() + bw.record_bytes("r", "ACGT", 0))
    struct.pack_into("<i", huge, len(bw.header_bytes()) + 4 + 16, 1 << 29)   # l_seq = 2^29 in an otherwise small record
    assert "longer than the limit" in _bad(exe, tmp_path, bw.bgzf_block(bytes(huge)) + bw.EOF_BLOCK)
