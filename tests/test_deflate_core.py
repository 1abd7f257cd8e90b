"""CPU test of the BGZF deflate core (metamaps_amd/csrc/mm_deflate.hpp, the same source as the device kernel, built for the host with g++
from tests/test_deflate_core.cpp): over a corpus every member is a sound BGZF block that zlib, Python's gzip and the project's own inflate
core read back to the input; the stored fallback keeps every member within 64 KiB; the 32 KiB window ends where it must; and on synthetic
mapping text the output is within 1.15 x of zlib level 1 on the same blocks with no block stored.  The driver also runs under
-fsanitize=address,undefined with the member and the token buffer in heap blocks of exactly their documented size."""
import os
import subprocess

import pytest

import deflate_corpus as dc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "test_deflate_core.cpp")


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("dc") / "t")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "asan_ubsan" else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", path, SRC], check=True, timeout=300)
    return path


def _deflate(exe, data, tmp_path):
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bgzf"
    inp.write_bytes(data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = [tuple(map(int, l.split())) for l in r.stdout.strip().split("\n")] if r.stdout.strip() else []
    return outp.read_bytes(), rows


def test_empty_input_gives_no_member(exe, tmp_path):
    comp, rows = _deflate(exe, b"", tmp_path)
    assert comp == b"" and rows == []


@pytest.mark.parametrize("case", dc.corpus(), ids=lambda c: c[0])
def test_corpus_round_trips(exe, tmp_path, case):
    name, data = case
    comp, rows = _deflate(exe, data, tmp_path)
    ms = dc.check_container(comp, data)
    assert len(rows) == len(ms)
    for m, (size, stored, status) in zip(ms, rows):
        assert size == len(m) <= 65536 and status == 0, (name, size, status)   # (status: the project's inflate core on the member)
        assert bool(stored) == dc.is_stored(m)
    if name == "random":
        assert all(dc.is_stored(m) for m in ms)
    if name == "period_32769":
        assert dc.is_stored(ms[0]) and len(comp) == 65280 + 31   # nothing is matched 32 769 bytes back: random bytes, stored
    if name == "one_repeated_byte":
        assert len(comp) < 1200
    if name in ("fastq", "mapping_text"):
        assert not any(dc.is_stored(m) for m in ms)


def test_window_edge(exe, tmp_path):
    """a 300-byte marker is found again exactly 32 768 bytes back (the filler between shares one hash slot, so the head table still holds
    the marker's positions), and not 32 769 bytes back"""
    at, beyond = dc.marker_pair()
    ca, _ = _deflate(exe, at, tmp_path)
    cb, _ = _deflate(exe, beyond, tmp_path)
    dc.check_container(ca, at); dc.check_container(cb, beyond)
    print(f"marker 32 768 back: {len(ca)} B, 32 769 back: {len(cb)} B")
    assert len(ca) < 700 and len(cb) > len(ca) + 250


def test_ratio_on_mapping_text(exe, tmp_path):
    """the condition of the feature: at most 1.15 x zlib level 1 on the same 65 280-byte blocks, no block stored"""
    data = dc.mapping_text(6 << 20)
    comp, rows = _deflate(exe, data, tmp_path)
    dc.check_container(comp, data)
    z1 = dc.zlib1_size(data)
    print(f"mapping text {len(data)} B: core {len(comp)} B ({len(data) / len(comp):.3f} x), zlib level 1 {z1} B ({len(data) / z1:.3f} x), core / zlib1 {len(comp) / z1:.4f}")
    assert not any(stored for _, stored, _ in rows)
    assert len(comp) <= dc.RATIO_BOUND * z1, (len(comp), z1)


def test_output_is_a_function_of_the_block_alone(exe, tmp_path):
    """a block's member does not depend on what stands before it in the input"""
    a, b = dc.mapping_text(dc.BLOCK_IN, seed=8), dc.mapping_text(dc.BLOCK_IN + 500, seed=9)
    ca, _ = _deflate(exe, a, tmp_path)
    cb, _ = _deflate(exe, b, tmp_path)
    cab, _ = _deflate(exe, a + b, tmp_path)
    assert cab == ca + cb
