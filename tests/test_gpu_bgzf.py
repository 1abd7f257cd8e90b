"""BGZF inflate on the device (mm_bgzf_inflate, metamaps_amd/csrc/mm_inflate.hip): one batch of many mixed blocks inflates to zlib's bytes,
a batch with corrupt blocks among good ones gets every status right and leaves the bad blocks' output untouched; and the CLI writes the
same files for bgzip FASTQ as for the plain FASTQ, and for BAM under device inflate as under host inflate (MM_BGZF_HOST_INFLATE=1), with
the host path's error for a corrupt block.  Fixtures: tests/bgzf_corpus.py and tests/bam_writer.py."""
import gzip
import os
import random
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bam_writer as bw
import bgzf_corpus as bc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "metamaps_amd", "csrc", "metamaps")


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def test_batch_of_mixed_blocks_equals_zlib(ctx):
    cases = bc.good_cases()
    rng = random.Random(5)
    blocks = [c for c in cases for _ in range(3)]                 # many blocks: more than one per workgroup of the grid
    for i in range(600):
        d = bc.fastq_text(rng, rng.choice([0, 1, 17, 1000, 30000, 65280]))
        blocks.append((f"fq{i}", bw.bgzf_block(d, level=rng.choice([1, 6, 9])), d, 0))
    rng.shuffle(blocks)
    out, st = ctx.bgzf_inflate([b for _, b, _, _ in blocks])
    assert list(st) == [0] * len(blocks)
    want = b"".join(d for _, _, d, _ in blocks)
    assert bytes(out) == want
    for _, b, d, _ in blocks[:40]:
        xlen = struct.unpack_from("<H", b, 10)[0]
        assert zlib.decompress(b[12 + xlen:-8], -15) == d


def test_statuses_of_a_batch_with_corrupt_blocks(ctx):
    good, bad = bc.good_cases(), bc.corrupt_cases()
    blocks, want = [], []
    for i, (_, b, d, _) in enumerate(good):
        blocks.append(b); want.append((0, d))
        if i < len(bad):
            blocks.append(bad[i][1]); want.append((bad[i][2], None))
    # every block gets its own output range (ISIZE when readable, else nothing), filled with a marker beforehand
    sizes = [len(d) if d is not None else (int.from_bytes(b[-4:], "little") if len(b) >= 26 and int.from_bytes(b[-4:], "little") <= 65536 else 0)
             for b, (_, d) in zip(blocks, want)]
    off = np.zeros(len(blocks), dtype=np.int64)
    off[1:] = np.cumsum(np.array(sizes[:-1], dtype=np.int64) + 5)
    cap = int(off[-1] + sizes[-1] + 5)
    from metamaps_amd import capi
    import ctypes as C
    comp = b"".join(blocks)
    cl = np.array([len(b) for b in blocks], dtype=np.int32)
    co = np.zeros(len(blocks), dtype=np.int64); co[1:] = np.cumsum(cl[:-1])
    out = bytearray(b"\xa5" * cap)
    status = np.full(len(blocks), -1, dtype=np.int32)
    rc = capi.lib().mm_bgzf_inflate(ctx.h, comp, len(comp), co.ctypes.data, cl.ctypes.data, len(blocks),
                                    C.cast((C.c_uint8 * cap).from_buffer(out), C.c_void_p), cap, off.ctypes.data, status.ctypes.data)
    assert rc == capi.MM_ERR_DATA
    for i, ((w, d), s) in enumerate(zip(want, status)):
        if w is None:
            assert s != 0, i
        else:
            assert s == w, (i, s, w)
        seg = bytes(out[off[i]:off[i] + sizes[i] + 5])
        if d is not None:
            assert seg == d + b"\xa5" * 5, i
        else:
            assert seg == b"\xa5" * (sizes[i] + 5), i                   # a failed block writes nothing


def test_bad_arguments(ctx):
    from metamaps_amd import capi
    import ctypes as C
    L = capi.lib()
    blk = bw.bgzf_block(b"hello world" * 10)
    co, cl, oo = np.zeros(1, np.int64), np.array([len(blk)], np.int32), np.zeros(1, np.int64)
    out = (C.c_uint8 * 200)()
    assert L.mm_bgzf_inflate(ctx.h, blk, len(blk), co.ctypes.data, cl.ctypes.data, 1, out, 200, oo.ctypes.data, None) == 0
    assert bytes(out)[:110] == b"hello world" * 10
    assert L.mm_bgzf_inflate(ctx.h, blk, len(blk), co.ctypes.data, cl.ctypes.data, 1, out, 109, oo.ctypes.data, None) == -1   # ISIZE does not fit
    cl2 = np.array([len(blk) + 1], np.int32)
    assert L.mm_bgzf_inflate(ctx.h, blk, len(blk), co.ctypes.data, cl2.ctypes.data, 1, out, 200, oo.ctypes.data, None) == -1  # outside comp
    assert L.mm_bgzf_inflate(ctx.h, blk, len(blk), co.ctypes.data, cl.ctypes.data, 0, out, 200, oo.ctypes.data, None) == 0    # nothing to do


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
SUFFIXES = ("", ".meta", ".meta.unmappedReadsLengths", ".parameters")
CLASSIFY_SUFFIXES = (".EM", ".EM.reads2Taxon", ".EM.reads2Taxon.krona", ".EM.WIMP", ".EM.lengthAndIdentitiesPerMappingUnit", ".EM.contigCoverage", ".EM.evidenceUnknownSpecies")
HOST = {"MM_BGZF_HOST_INFLATE": "1"}
DEV = {"MM_BAM_DEVICE_INFLATE": "1"}                               # (BAM's default is host inflate; bgzip text's is the device)


def _bgzip(src, dst, block_bytes):
    """what bgzip writes for src (blocks cut wherever block_bytes falls, mid-record), with the EOF block"""
    bw.write_bgzf(dst, open(src, "rb").read(), block_bytes)
    return dst


def _gzip(src, dst):
    """what gzip writes for src: one DEFLATE stream, no BGZF blocks"""
    with gzip.open(dst, "wb") as f:
        f.write(open(src, "rb").read())
    return dst


def _fastq_records(path):
    out = []
    with open(path) as f:
        while True:
            h = f.readline()
            if not h:
                break
            s = f.readline().strip(); f.readline(); f.readline()
            out.append((h[1:].split()[0], s.upper()))
    return out


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("bgzfcli")
    db = synth.make_db(str(d / "db"), n_genomes=10, genome_len=60_000, seed=7)
    r1 = synth.make_reads(db, str(d / "r1.fq"), n_reads=220, read_len=3000, seed=3)["path"]
    r2 = synth.make_reads(db, str(d / "r2.fq"), n_reads=90, read_len=2500, seed=4)["path"]
    fa = str(d / "r3.fa")                                          # FASTA with wrapped lines and lower case, as kseq reads it
    with open(fa, "w") as f:
        for i, (n, s) in enumerate(_fastq_records(r2)):
            s = s.lower() if i % 3 == 0 else s
            f.write(f">{n} extra words\n" + "".join(s[k:k + 61] + "\n" for k in range(0, len(s), 61)))
    recs = [(n, s, 0x10 if i % 2 else 0) for i, (n, s) in enumerate(_fastq_records(r1))]
    bw.write_bam(str(d / "r1.bam"), recs, block_bytes=20000)
    return {"db": db, "dir": d, "r1": r1, "r2": r2, "fa": fa, "bam": str(d / "r1.bam"),
            "r1z": _bgzip(r1, str(d / "r1z.fq.gz"), 20000), "r2z": _bgzip(r2, str(d / "r2z.fq.gz"), 777),
            "faz": _bgzip(fa, str(d / "r3z.fa.gz"), 333), "r1g": _gzip(r1, str(d / "r1g.fq.gz"))}


def _map(args, env=None):
    p = subprocess.run([CLI] + args, capture_output=True, timeout=900, env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p


def _same_files(a, b, subst, suffixes):
    for suf in suffixes:
        x = open(a + suf).read()
        y = open(b + suf).read()
        for u, v in subst:
            x = x.replace(u, v)
        assert x == y, (suf, a, b)


@pytest.mark.parametrize("mode", ["all", "best"])
@pytest.mark.parametrize("which", [("r1z", "r1"), ("r2z", "r2"), ("faz", "fa")])
def test_cli_map_directly_bgzip_equals_plain(data, tmp_path, mode, which):
    db, z, plain = data["db"], data[which[0]], data[which[1]]
    flags = ["--all"] if mode == "all" else []
    _map(["mapDirectly"] + flags + ["-r", db.fasta, "-q", plain, "-o", str(tmp_path / "plain")])
    p = _map(["mapDirectly"] + flags + ["-r", db.fasta, "-q", z, "-o", str(tmp_path / "z")], {"MM_CLI_TIMING": "1"})
    assert b"bgzip reader" in p.stderr                              # (the device path was taken, not zlib's)
    assert os.path.getsize(str(tmp_path / "z")) > 1000
    _same_files(str(tmp_path / "z"), str(tmp_path / "plain"), [(z, plain), (str(tmp_path / "z"), str(tmp_path / "plain"))], SUFFIXES)


@pytest.mark.parametrize("which", ["r1z", "bam"])
def test_cli_device_inflate_equals_host_inflate(data, tmp_path, which):
    db, f = data["db"], data[which]
    _map(["mapDirectly", "--all", "-r", db.fasta, "-q", f, "-o", str(tmp_path / "dev")], DEV)
    _map(["mapDirectly", "--all", "-r", db.fasta, "-q", f, "-o", str(tmp_path / "host")], HOST)
    _same_files(str(tmp_path / "dev"), str(tmp_path / "host"), [(str(tmp_path / "dev"), str(tmp_path / "host"))], SUFFIXES)


def test_cli_map_against_index_bgzip_equals_plain(data, tmp_path):
    db, z, plain = data["db"], data["r1z"], data["r1"]
    _map(["index", "-r", db.fasta, "-i", str(tmp_path / "idx"), "--maxmemory-bytes", "1000000"])
    _map(["mapAgainstIndex", "--all", "-i", str(tmp_path / "idx"), "-q", plain, "-o", str(tmp_path / "plain")])
    _map(["mapAgainstIndex", "--all", "-i", str(tmp_path / "idx"), "-q", z, "-o", str(tmp_path / "z")])
    _same_files(str(tmp_path / "z"), str(tmp_path / "plain"), [(z, plain), (str(tmp_path / "z"), str(tmp_path / "plain"))], SUFFIXES)


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_cli_then_classify_mixed_list(data, tmp_path, devices):
    """a comma list of bgzip FASTQ, BAM, plain FASTA and plain gzip FASTQ — every kind of query file the reader knows, each ending its file for the
    writer —, mapped and classified in one process, writes the files of the all-plain list; and the same list under host inflate writes them too"""
    db = data["db"]
    dev = ["--devices", devices, "--em-host-reduce"] if devices else []
    common = ["--then-classify", db.dir, "--minreads", "3"] + dev
    plain = [data["r2"], data["r1"], data["fa"], data["r1"]]
    mixed = [data["r2z"], data["bam"], data["fa"], data["r1g"]]
    outs = {k: [str(tmp_path / f"{k}_{i}") for i in range(4)] for k in ("plain", "dev", "host")}
    _map(["mapDirectly", "--all", "-r", db.fasta, "-q", ",".join(plain), "-o", ",".join(outs["plain"])] + common)
    _map(["mapDirectly", "--all", "-r", db.fasta, "-q", ",".join(mixed), "-o", ",".join(outs["dev"])] + common, dict(DEV, MM_CLI_BATCH_READS="64"))
    _map(["mapDirectly", "--all", "-r", db.fasta, "-q", ",".join(mixed), "-o", ",".join(outs["host"])] + common, HOST)
    for k in ("dev", "host"):
        subst = list(zip(mixed, plain)) + list(zip(outs[k], outs["plain"]))
        for a, b in zip(outs[k], outs["plain"]):
            _same_files(a, b, subst, SUFFIXES + CLASSIFY_SUFFIXES)
    assert os.path.getsize(outs["dev"][0] + ".EM.WIMP") > 200


def _blocks(raw):
    out, i = [], 0
    while i < len(raw):
        bs = struct.unpack_from("<H", raw, i + 16)[0] + 1
        out.append((i, bs)); i += bs
    return out


@pytest.mark.parametrize("damage", ["crc", "deflate"])
def test_cli_corrupt_bam_block_error_matches_host(data, tmp_path, damage):
    db, bam = data["db"], data["bam"]
    raw = bytearray(open(bam, "rb").read())
    off, bs = _blocks(bytes(raw))[3]
    if damage == "crc":
        raw[off + bs - 8] ^= 0xFF
    else:
        for k in range(40):
            raw[off + 18 + 200 + k] ^= 0x5A
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(raw))
    runs = {}
    for k, env in (("dev", DEV), ("host", HOST)):
        runs[k] = subprocess.run([CLI, "mapDirectly", "-r", db.fasta, "-q", bad, "-o", str(tmp_path / k)], capture_output=True, timeout=900,
                                 env=dict(os.environ, **(env or {})))
    assert runs["dev"].returncode == runs["host"].returncode != 0
    line = lambda p: [l for l in p.stderr.decode().split("\n") if "BGZF" in l]
    assert line(runs["dev"]) == line(runs["host"]) and len(line(runs["dev"])) == 1, (runs["dev"].stderr[-800:], runs["host"].stderr[-800:])
    assert f"corrupt BGZF block at byte {off}" in line(runs["dev"])[0]


def test_cli_corrupt_bgzip_block_is_an_error(data, tmp_path):
    """(zlib's gzread path ends such a file silently where the damage starts; the device path names the block and fails)"""
    db, z = data["db"], data["r1z"]
    raw = bytearray(open(z, "rb").read())
    off, bs = _blocks(bytes(raw))[2]
    raw[off + bs - 8] ^= 0xFF
    bad = str(tmp_path / "bad.fq.gz")
    open(bad, "wb").write(bytes(raw))
    p = subprocess.run([CLI, "mapDirectly", "-r", db.fasta, "-q", bad, "-o", str(tmp_path / "x")], capture_output=True, timeout=900)
    assert p.returncode != 0 and f"corrupt BGZF block at byte {off} (CRC mismatch)".encode() in p.stderr, p.stderr[-800:]
