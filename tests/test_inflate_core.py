"""CPU test of the BGZF decode core (metamaps_amd/csrc/mm_inflate.hpp, the same source as the device kernel, built for the host with g++ from
tests/test_inflate_core.cpp): every DEFLATE form zlib writes, and hand-built ones it never writes, inflate to zlib's bytes; every corrupt
block gets its status.  The driver also runs under -fsanitize=address,undefined, with each block and its output in buffers of exactly their
size, so a read or write outside them fails the run."""
import os
import struct
import subprocess
import zlib

import pytest

import bgzf_corpus as bc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "test_inflate_core.cpp")


def _build(path, sanitize):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", path, SRC], check=True, timeout=300)
    return path


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def exe(request, tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("ic") / "t"), request.param == "asan_ubsan")


def _run(exe, blocks, tmp_path):
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(bc.pack(blocks))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    sts = [tuple(map(int, l.split())) for l in r.stdout.strip().split("\n")]
    raw, outs, i = outp.read_bytes(), [], 0
    while i < len(raw):
        (n,) = struct.unpack_from("<I", raw, i)
        outs.append(raw[i + 4:i + 4 + n]); i += 4 + n
    return sts, outs


def test_good_blocks_match_zlib(exe, tmp_path):
    cases = bc.good_cases()
    sts, outs = _run(exe, [b for _, b, _, _ in cases], tmp_path)
    assert len(sts) == len(cases) and len(outs) == len(cases)
    for (name, blk, data, _), (st, isize), got in zip(cases, sts, outs):
        assert st == bc.OK, (name, st)
        xlen = struct.unpack_from("<H", blk, 10)[0]
        assert got == data == zlib.decompress(blk[12 + xlen:-8], -15), name
        assert isize == len(data), name


def test_corrupt_blocks_get_their_status(exe, tmp_path):
    cases = bc.corrupt_cases()
    sts, outs = _run(exe, [b for _, b, _ in cases], tmp_path)
    assert outs == []
    for (name, _, want), (st, _) in zip(cases, sts):
        if want is None:
            assert st != bc.OK, name
        else:
            assert st == want, (name, st, want)


def test_corrupt_blocks_fail_in_zlib_too(tmp_path):
    """the corpus' corrupt blocks are ones zlib (the host path's bam::bgzf_inflate) rejects as well, and the good ones it accepts"""
    for name, blk, want in bc.corrupt_cases():
        if want == bc.BAD_HEADER:
            continue
        xlen = struct.unpack_from("<H", blk, 10)[0]
        crc, isize = struct.unpack("<II", blk[-8:])
        try:
            d = zlib.decompressobj(-15)
            out = d.decompress(blk[12 + xlen:-8], 65536 + 1)
            ok = d.eof and len(out) == isize and (zlib.crc32(out) & 0xFFFFFFFF) == crc
        except zlib.error:
            ok = False
        assert not ok, name


def test_mixed_batch_keeps_order(exe, tmp_path):
    good, bad = bc.good_cases(), bc.corrupt_cases()
    blocks, want = [], []
    for i, (n, b, d, _) in enumerate(good):
        blocks.append(b); want.append((bc.OK, d))
        if i < len(bad):
            blocks.append(bad[i][1]); want.append((bad[i][2], None))
    sts, outs = _run(exe, blocks, tmp_path)
    assert [o for s, o in want if s == bc.OK] == outs
    for (w, _), (st, _) in zip(want, sts):
        assert (st == bc.OK) == (w == bc.OK)
