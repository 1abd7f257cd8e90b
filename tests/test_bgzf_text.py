"""CPU test of bgzip FASTA/FASTQ in the CLI's reader (tests/test_bgzf_text.cpp over metamaps_amd/csrc/host/seq_reader.hpp and bam_reader.hpp):
the record parse over the inflated segments of a BGZF file (the path the CLI takes, the device inflating the segments) gives exactly the
records zlib's gzread path gives for the same file — kseq's quirks included, with records that span blocks and segments — and bgzip text
is told from BAM, plain gzip and plain text by content."""
import gzip
import os
import random
import subprocess

import pytest

import bam_writer as bw

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("bt") / "t")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-o", e, os.path.join(HERE, "test_bgzf_text.cpp"), "-lz"], check=True, timeout=300)
    return e


def _text(rng, kind, n):
    out = []
    for i in range(n):
        L = rng.choice([0, 1, 60, 61, 500, 3000]) + rng.randrange(0, 30)
        s = "".join(rng.choice("ACGTacgtNRY") for _ in range(L))
        if kind == "fasta":
            out.append(f">r{i} desc {i}\n" + "".join(s[k:k + 61] + "\n" for k in range(0, len(s), 61)))
        elif kind == "fastq":
            out.append(f"@r{i}\n{s}\n+\n{'I' * L}\n")
        else:                                                     # kseq's odd corners: wrapped FASTQ, '+name' lines, CRLF, blank lines,
            q = "".join(rng.choice("!#5?IJ~") for _ in range(L))  # '@' in qualities, a header without a newline before it
            v = i % 6
            if v == 0:
                out.append(f"@r{i} x\n" + "\n".join(s[k:k + 50] for k in range(0, len(s), 50)) + f"\n+r{i}\n" + "\n".join(q[k:k + 70] for k in range(0, len(q), 70)) + "\n")
            elif v == 1:
                out.append(f"@r{i}\r\n{s}\r\n+\r\n{q}\r\n")
            elif v == 2:
                out.append(f"\n\n>r{i}\n{s}\n\n")
            elif v == 3:
                out.append(f"@r{i}\n{s}\n+\n{q}")
            else:
                out.append(f"@r{i}\t tab\n{s}\n+\n{q}\n")
    return "".join(out).encode()


def _run(exe, *args):
    p = subprocess.run([exe, *args], capture_output=True, timeout=600)
    return p.returncode, p.stdout


@pytest.mark.parametrize("kind", ["fasta", "fastq", "quirks"])
@pytest.mark.parametrize("block", [7, 333, 65280])
def test_bgzf_segments_equal_gzread(exe, tmp_path, kind, block):
    rng = random.Random(f"{kind}{block}")
    data = _text(rng, kind, 400)
    path = str(tmp_path / "r.gz")
    bw.write_bgzf(path, data, block)                               # (block 7: segments of 1024 blocks end mid-record)
    a, b = _run(exe, "gz", path), _run(exe, "bgzf", path)
    assert a[0] == 0 and a == b
    assert a[1].count(b"\n") > 100


def test_empty_and_eof_only(exe, tmp_path):
    path = str(tmp_path / "e.gz")
    open(path, "wb").write(bw.EOF_BLOCK)
    assert _run(exe, "gz", path) == _run(exe, "bgzf", path) == (0, b"end\n")


def test_detect(exe, tmp_path):
    data = _text(random.Random(1), "fastq", 20)
    p = {k: str(tmp_path / k) for k in ("bgzf", "gz", "plain", "bam")}
    bw.write_bgzf(p["bgzf"], data, 1000)
    open(p["gz"], "wb").write(gzip.compress(data))
    open(p["plain"], "wb").write(data)
    bw.write_bam(p["bam"], [("a", "ACGT", 0)])
    _, out = _run(exe, "detect", p["bgzf"], p["gz"], p["plain"], p["bam"])
    assert out.decode().split("\n")[:4] == ["1 0", "0 0", "0 0", "1 1"]


def test_corrupt_block_is_an_error(exe, tmp_path):
    data = _text(random.Random(2), "fastq", 50)
    path = str(tmp_path / "c.gz")
    bw.write_bgzf(path, data, 1000)
    raw = bytearray(open(path, "rb").read())
    bs = int.from_bytes(raw[16:18], "little") + 1
    raw[bs + (int.from_bytes(raw[bs + 16:bs + 18], "little") + 1) - 8] ^= 1     # the second block's CRC
    open(path, "wb").write(bytes(raw))
    rc, out = _run(exe, "bgzf", path)
    assert rc == 2 and out.endswith(f"error: corrupt BGZF block at byte {bs} (CRC mismatch)\n".encode())
