"""CPU test of the plain gzip decoder (metamaps_amd/csrc/mm_gzip.hpp — the same source as the device kernels — on its host backend, built
with g++ from tests/test_gzip_core.cpp): on every stream of gzip_corpus the output equals zlib's at chunk sizes from 1 KiB to the whole file
and with the stream fed in pieces cut at random offsets; the speculation is accepted where it should be; every corrupt stream fails with a
compressed byte offset.  The driver also runs under -fsanitize=address,undefined with every piece fed in a buffer of exactly its size."""
import os
import subprocess
import zlib

import pytest

import gzip_corpus as gc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "test_gzip_core.cpp")


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gz") / "t")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "asan_ubsan" else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", path, SRC], check=True, timeout=300)
    return path


def run(exe, tmp_path, comp, chunk, segment=1 << 28, seed=0):
    inp, outp = tmp_path / "in.gz", tmp_path / "out.bin"
    inp.write_bytes(comp)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(inp), str(outp), str(chunk), str(segment), str(seed)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    rc, off, chunks, acc, redo, skip, members = map(int, lines[0].split())
    return dict(rc=rc, off=off, chunks=chunks, accepted=acc, redone=redo, skipped=skip, members=members,
                msg=lines[1] if len(lines) > 1 else "", out=outp.read_bytes())


CASES = gc.good_cases()


@pytest.mark.parametrize("name,comp,data", CASES, ids=[c[0] for c in CASES])
def test_matches_zlib_at_every_chunk_size(exe, tmp_path, name, comp, data):
    d = zlib.decompressobj(31)
    want = d.decompress(comp)
    while d.unused_data and d.unused_data[:2] == b"\x1f\x8b":     # concatenated members, as gzread reads them
        rest = d.unused_data
        d = zlib.decompressobj(31)
        want += d.decompress(rest)
    assert want == data, name
    for chunk, segment, seed in ((1024, 1 << 28, 0), (4096, 1 << 28, 0), (16384, 1 << 28, 0), (len(comp) + 1, 1 << 28, 0),
                                 (2048, 16384, 3), (4096, 40000, 17), (1024, 1 << 28, 29)):
        r = run(exe, tmp_path, comp, chunk, segment, seed)
        assert r["rc"] == 0, (name, chunk, segment, seed, r["msg"])
        assert r["out"] == data, (name, chunk, segment, seed)
        assert r["chunks"] == r["accepted"] + r["redone"] + r["skipped"]


@pytest.mark.parametrize("k", [1, 3, 5, 8, 9, 12, 20])
def test_feed_cut_inside_the_trailer_of_a_final_stored_block(exe, tmp_path, k):
    """a member whose non-empty final stored block reaches the end of a feed that is not the last, so that its trailer arrives with the
    next feed: the stream still decodes, whatever the chunk and segment sizes"""
    import random
    fq = gc.fastq_text(random.Random(8), 200_000)
    comp = gc.member(gc.stored_deflate(fq), fq)
    for chunk, segment in ((1024, 1024), (1024, 4096), (1024, 20000), (4096, 1 << 28)):
        r = run(exe, tmp_path, comp, chunk, segment, f"c{len(comp) - k}")
        assert r["rc"] == 0, (k, chunk, segment, r["msg"])
        assert r["out"] == fq, (k, chunk, segment)
    two = gc.member(gc.stored_deflate(fq), fq) + gc.gz(fq[:5000], 6)    # ... and the next member follows in the second feed
    r = run(exe, tmp_path, two, 1024, 4096, f"c{len(comp) - k}")
    assert r["rc"] == 0 and r["out"] == fq + fq[:5000] and r["members"] == 2, (k, r["msg"])


def test_speculation_is_accepted_on_level6_fastq(exe, tmp_path):
    import random
    fq = gc.fastq_text(random.Random(3), 1_500_000)
    comp = gc.gz(fq, 6)
    # zlib closes a level-6 block every 16 Ki symbols, about 30 KB of this FASTQ compressed: with chunks larger than a block every chunk
    # holds a block start, and at least 90 % of all chunks must be accepted
    r = run(exe, tmp_path, comp, 65536)
    assert r["rc"] == 0 and r["out"] == fq
    assert r["chunks"] >= len(comp) // 65536
    assert r["accepted"] >= 0.9 * r["chunks"], r
    # with 16 KiB chunks about half of them lie inside one block and have no block start to speculate from (they are covered by the chunk
    # before: "skipped"); of those that hold one, at least 90 % must be accepted
    r = run(exe, tmp_path, comp, 16384)
    assert r["rc"] == 0 and r["out"] == fq
    assert r["chunks"] >= len(comp) // 16384
    assert r["accepted"] >= 0.9 * (r["accepted"] + r["redone"]), r


def test_fixed_huffman_stream_decodes_sequentially_and_exactly(exe, tmp_path):
    import random
    import zlib as z
    fq = gc.fastq_text(random.Random(4), 300_000)
    r = run(exe, tmp_path, gc.gz(fq, 6, z.Z_FIXED), 4096)
    assert r["rc"] == 0 and r["out"] == fq
    assert r["redone"] >= 1


CORRUPT = gc.corrupt_cases()


@pytest.mark.parametrize("name,comp,span", CORRUPT, ids=[c[0] for c in CORRUPT])
def test_corrupt_stream_is_an_error_with_its_offset(exe, tmp_path, name, comp, span):
    for chunk, segment, seed in ((4096, 1 << 28, 0), (len(comp) + 1, 1 << 28, 0), (2048, 16384, 5)):
        r = run(exe, tmp_path, comp, chunk, segment, seed)
        assert r["rc"] != 0, (name, chunk)
        assert span[0] <= r["off"] <= span[1], (name, chunk, r["off"], span, r["msg"])
        assert f"offset {r['off']}" in r["msg"]
