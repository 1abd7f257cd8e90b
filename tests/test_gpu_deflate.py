"""BGZF deflate on the device (mm_bgzf_deflate, metamaps_amd/csrc/mm_deflate.hip) through capi.py: over the corpus of
tests/deflate_corpus.py the device writes, byte for byte, what the host build of the same core (tests/test_deflate_core.cpp) writes; the
members are sound BGZF that zlib, Python's gzip and mm_bgzf_inflate read back; 8 MiB and 200 MiB of mapping text (many blocks per
workgroup, the pinned staging growing); the ratio condition on mapping text; MM_DEFLATE_HOST=1; argument errors."""
import os
import struct
import subprocess

import pytest

import deflate_corpus as dc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("dch") / "t")
    subprocess.run(["g++", "-std=c++17", "-O2", "-o", path, os.path.join(HERE, "test_deflate_core.cpp")], check=True, timeout=300)
    return path


def _host(host_exe, data, tmp_path):
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bgzf"
    inp.write_bytes(data)
    subprocess.run([host_exe, str(inp), str(outp)], check=True, capture_output=True, timeout=900)
    return outp.read_bytes()


def _inflate_on_device(ctx, comp):
    ms = dc.members(comp)
    out, st = ctx.bgzf_inflate(ms)
    assert list(st) == [0] * len(ms)
    return bytes(out)


def test_empty_input(ctx):
    comp, n = ctx.bgzf_deflate(b"")
    assert comp == b"" and n == 0


@pytest.mark.parametrize("case", dc.corpus(), ids=lambda c: c[0])
def test_device_equals_host_core_and_round_trips(ctx, host_exe, tmp_path, case):
    name, data = case
    comp, n = ctx.bgzf_deflate(data)
    ms = dc.check_container(comp, data)
    assert n == len(ms)
    assert comp == _host(host_exe, data, tmp_path), name          # byte-identical to the host build of the core
    assert _inflate_on_device(ctx, comp) == data


def test_window_edge_pair_equals_host_core(ctx, host_exe, tmp_path):
    for data in dc.marker_pair():
        comp, _ = ctx.bgzf_deflate(data)
        assert comp == _host(host_exe, data, tmp_path)


def test_8_mib_of_mapping_text_and_the_ratio(ctx, host_exe, tmp_path):
    data = dc.mapping_text(8 << 20)
    comp, n = ctx.bgzf_deflate(data)
    ms = dc.check_container(comp, data)
    assert n == len(ms) == (len(data) + dc.BLOCK_IN - 1) // dc.BLOCK_IN
    assert comp == _host(host_exe, data, tmp_path)
    assert _inflate_on_device(ctx, comp) == data
    z1 = dc.zlib1_size(data)
    print(f"mapping text {len(data)} B: device {len(comp)} B ({len(data) / len(comp):.3f} x), zlib level 1 {z1} B, device / zlib1 {len(comp) / z1:.4f}")
    assert not any(dc.is_stored(m) for m in ms)
    assert len(comp) <= dc.RATIO_BOUND * z1


def test_200_mib_of_mapping_text(ctx):
    import gzip
    import zlib
    piece = dc.mapping_text(10 << 20, seed=12)
    data = b"".join(piece[i:] + piece[:i] for i in range(0, 20 * 997, 997))   # 200 MiB, no two blocks alike
    assert len(data) == 200 << 20
    comp, n = ctx.bgzf_deflate(data)
    assert n == (len(data) + dc.BLOCK_IN - 1) // dc.BLOCK_IN
    ms = dc.members(comp)
    assert len(ms) == n and all(struct.unpack("<I", m[-4:])[0] <= dc.BLOCK_IN for m in ms)
    assert zlib.crc32(gzip.decompress(comp + dc.EOF_BLOCK)) == zlib.crc32(data)
    assert _inflate_on_device(ctx, comp) == data
    comp2, _ = ctx.bgzf_deflate(data[:8 << 20])                   # a block's member does not depend on the call that carries it
    assert comp.startswith(comp2[:len(b"".join(dc.members(comp2)[:-1]))])


def test_host_switch_inflates_to_the_same_text(ctx):
    data = dc.mapping_text(3 << 20, seed=4) + bytes(range(256)) * 300
    os.environ["MM_DEFLATE_HOST"] = "1"
    try:
        comp, n = ctx.bgzf_deflate(data)
    finally:
        del os.environ["MM_DEFLATE_HOST"]
    dc.check_container(comp, data)
    dev, n2 = ctx.bgzf_deflate(data)
    assert n == n2 and dev != comp                                # (zlib's bytes, not the core's)
    assert _inflate_on_device(ctx, comp) == data


def test_argument_errors(ctx):
    import ctypes as C
    from metamaps_amd import capi
    L = capi.lib()
    assert L.mm_bgzf_deflate_bound(0) == 0 and L.mm_bgzf_deflate_bound(1) == 32
    assert L.mm_bgzf_deflate_bound(65280) == 65280 + 31 and L.mm_bgzf_deflate_bound(65281) == 65281 + 62
    with pytest.raises(capi.MMError) as e:
        ctx.bgzf_deflate(b"x" * 1000, out_cap=1000 + 30)
    assert "mm_bgzf_deflate_bound" in str(e.value)
    nbytes, nblocks = C.c_int64(), C.c_int32()
    buf = (C.c_uint8 * 64)()
    assert L.mm_bgzf_deflate(ctx.h, None, 5, buf, 64, C.byref(nbytes), C.byref(nblocks)) == capi.MM_ERR_ARG
    assert L.mm_bgzf_deflate(ctx.h, b"hello", 5, None, 64, C.byref(nbytes), C.byref(nblocks)) == capi.MM_ERR_ARG
    assert L.mm_bgzf_deflate(ctx.h, b"hello", 5, buf, 64, None, C.byref(nblocks)) == capi.MM_ERR_ARG
    assert L.mm_bgzf_deflate(ctx.h, b"hello", 5, buf, 64, C.byref(nbytes), None) == capi.MM_ERR_ARG
    assert L.mm_bgzf_deflate(None, b"hello", 5, buf, 64, C.byref(nbytes), C.byref(nblocks)) == capi.MM_ERR_ARG
