"""Plain gzip inflated on the device (mm_gzip_*, metamaps_amd/csrc/mm_gzip.hip): through capi, every stream of tests/gzip_corpus.py inflates
to zlib's bytes at several chunk and segment sizes, with the same chunk counters as the host build of the same driver (tests/test_gzip_core.cpp),
and every corrupt stream fails with its offset; through the CLI, a plain gzip query (one member, two members, trailing garbage) or reference
writes the files of the uncompressed input and of zlib's reader (MM_GZIP_HOST_INFLATE=1), and a corrupt one is an error with its offset."""
import gzip
import os
import random
import re
import shutil
import subprocess
import zlib

import pytest

import gzip_corpus as gc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "metamaps_amd", "csrc", "metamaps")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gzh") / "t")
    subprocess.run(["g++", "-std=c++17", "-O2", "-o", path, os.path.join(HERE, "test_gzip_core.cpp")], check=True, timeout=300)
    return path


CASES = gc.good_cases()


@pytest.mark.parametrize("name,comp,data", CASES, ids=[c[0] for c in CASES])
def test_device_equals_zlib(ctx, name, comp, data, tmp_path):
    rng = random.Random(len(comp))
    for chunk, segment, pieces in ((1024, 0, None), (4096, 0, None), (len(comp) + 1, 0, None), (2048, 16384, None),
                                   (4096, 40000, [rng.randrange(1, 30000) for _ in range(40)])):
        out, st = ctx.gzip_inflate(comp, chunk, segment, pieces)
        assert out == data, (name, chunk, segment)
        assert st["chunks"] == st["accepted"] + st["redone"] + st["skipped"]


@pytest.mark.parametrize("name,comp,data", CASES[:8] + CASES[-6:], ids=[c[0] for c in CASES[:8] + CASES[-6:]])
def test_device_equals_host_build_with_its_counters(ctx, host_exe, name, comp, data, tmp_path):
    inp, outp = tmp_path / "in.gz", tmp_path / "out.bin"
    inp.write_bytes(comp)
    for chunk, segment in ((2048, 1 << 28), (8192, 30000)):
        r = subprocess.run([host_exe, str(inp), str(outp), str(chunk), str(segment), "0"], capture_output=True, text=True, timeout=300)
        rc, _, chunks, acc, redo, skip, members = map(int, r.stdout.split("\n")[0].split())
        out, st = ctx.gzip_inflate(comp, chunk, segment)
        assert rc == 0 and out == outp.read_bytes() == data
        assert (st["chunks"], st["accepted"], st["redone"], st["skipped"], st["members"]) == (chunks, acc, redo, skip, members), name


def test_speculation_runs_in_parallel_on_fastq(ctx):
    fq = gc.fastq_text(random.Random(3), 3_000_000)
    comp = gzip.compress(fq, 6)
    out, st = ctx.gzip_inflate(comp, 16384)
    assert out == fq
    assert st["accepted"] >= 0.9 * (st["accepted"] + st["redone"]) and st["accepted"] >= 40, st


@pytest.mark.parametrize("k", [1, 5, 8, 9])
def test_device_feed_cut_inside_the_trailer_of_a_final_stored_block(ctx, k):
    fq = gc.fastq_text(random.Random(8), 200_000)
    comp = gc.member(gc.stored_deflate(fq), fq) + gc.gz(fq[:5000], 6)
    cut = len(comp) - len(gc.gz(fq[:5000], 6)) - k
    for chunk, segment in ((1024, 1024), (1024, 20000), (4096, 0)):
        out, st = ctx.gzip_inflate(comp, chunk, segment, [cut])
        assert out == fq + fq[:5000] and st["members"] == 2, (k, chunk, segment)


CORRUPT = gc.corrupt_cases()


@pytest.mark.parametrize("name,comp,span", CORRUPT, ids=[c[0] for c in CORRUPT])
def test_corrupt_stream_is_data_error_with_offset(ctx, name, comp, span):
    from metamaps_amd import capi
    for chunk in (4096, len(comp) + 1):
        with pytest.raises(capi.MMError) as e:
            ctx.gzip_inflate(comp, chunk)
        assert e.value.status == capi.MM_ERR_DATA
        off = int(re.search(r"offset (\d+)", str(e.value)).group(1))
        assert span[0] <= off <= span[1], (name, off, span, str(e.value))


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
SUFFIXES = ("", ".meta", ".meta.unmappedReadsLengths", ".parameters")
CLASSIFY_SUFFIXES = (".EM", ".EM.reads2Taxon", ".EM.reads2Taxon.krona", ".EM.WIMP", ".EM.lengthAndIdentitiesPerMappingUnit", ".EM.contigCoverage", ".EM.evidenceUnknownSpecies")
CHUNK = {"MM_GZIP_CHUNK_BYTES": "65536"}
HOST = {"MM_GZIP_HOST_INFLATE": "1"}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("gzcli")
    db = synth.make_db(str(d / "db"), n_genomes=10, genome_len=60_000, seed=7)
    r1 = synth.make_reads(db, str(d / "r1.fq"), n_reads=400, read_len=3000, seed=3)["path"]
    raw = open(r1, "rb").read()
    cut = raw.index(b"\n@", len(raw) // 2) + 1
    out = {"db": db, "r1": r1}
    out["r1z"] = str(d / "r1z.fq.gz"); open(out["r1z"], "wb").write(gzip.compress(raw, 6))
    out["r1m"] = str(d / "r1m.fq.gz"); open(out["r1m"], "wb").write(gzip.compress(raw[:cut], 6) + gzip.compress(raw[cut:], 1))
    out["r1g"] = str(d / "r1g.fq.gz"); open(out["r1g"], "wb").write(gzip.compress(raw, 9) + b"trailing garbage\n" * 20)
    out["refz"] = str(d / "ref.fa.gz"); open(out["refz"], "wb").write(gzip.compress(open(db.fasta, "rb").read(), 6))
    return out


def _map(args, env=None):
    p = subprocess.run([CLI] + args, capture_output=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p


def _same_files(a, b, subst, suffixes):
    for suf in suffixes:
        x = open(a + suf).read()
        y = open(b + suf).read()
        for u, v in subst:
            x = x.replace(u, v)
        assert x == y, (suf, a, b)


@pytest.mark.parametrize("which", ["r1z", "r1m", "r1g", "refz"])
def test_cli_map_and_classify_gzip_equals_plain_and_zlib(data, tmp_path, which):
    db = data["db"]
    common = ["--all", "--then-classify", db.dir, "--minreads", "3"]
    ref, q = (data["refz"], data["r1"]) if which == "refz" else (db.fasta, data[which])
    _map(["mapDirectly", "-r", db.fasta, "-q", data["r1"], "-o", str(tmp_path / "plain")] + common)
    p = _map(["mapDirectly", "-r", ref, "-q", q, "-o", str(tmp_path / "dev")] + common, dict(CHUNK, MM_CLI_TIMING="1"))
    # (the phase line of the reader that took the device path: zlib's reader would write the same files)
    assert (b"reference gzip reader (device inflate" if which == "refz" else b"R gzip reader (device inflate") in p.stderr, p.stderr[-2000:]
    _map(["mapDirectly", "-r", ref, "-q", q, "-o", str(tmp_path / "host")] + common, HOST)
    assert os.path.getsize(str(tmp_path / "dev")) > 1000
    # (.parameters records referenceSize, the size of the -r file as given: compressed for a .fa.gz, as under zlib's reader)
    sufs = tuple(s for s in SUFFIXES + CLASSIFY_SUFFIXES if which != "refz" or s != ".parameters")
    for k in ("dev", "host"):
        subst = [(q, data["r1"]), (ref, db.fasta), (str(tmp_path / k), str(tmp_path / "plain"))]
        _same_files(str(tmp_path / k), str(tmp_path / "plain"), subst, sufs)
    _same_files(str(tmp_path / "dev"), str(tmp_path / "host"), [(str(tmp_path / "dev"), str(tmp_path / "host"))], SUFFIXES + CLASSIFY_SUFFIXES)


def test_cli_corrupt_gzip_is_an_error_with_offset(data, tmp_path):
    """(zlib's gzread path ends such a file silently somewhere before the damage; the device path fails and names the offset)"""
    raw = bytearray(open(data["r1z"], "rb").read())
    raw[-8] ^= 0xFF                                                # the CRC32
    bad = str(tmp_path / "bad.fq.gz")
    open(bad, "wb").write(bytes(raw))
    p = subprocess.run([CLI, "mapDirectly", "-r", data["db"].fasta, "-q", bad, "-o", str(tmp_path / "x")], capture_output=True, timeout=300,
                       env=dict(os.environ, **CHUNK))
    assert p.returncode != 0 and f"CRC32 mismatch at compressed byte offset {len(raw) - 8}".encode() in p.stderr, p.stderr[-800:]
