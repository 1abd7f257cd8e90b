"""`mapDirectly --bam-sorted`: PREFIX.sorted.bam and PREFIX.sorted.bam.bai beside the outputs of the same run without the flag, which stay byte for byte.
The sorted file's records are the stable sort of PREFIX.bam's by (refID, pos), its header the one of PREFIX.bam with SO:coordinate, its members of 65 280
bytes, its index the bytes tests/bai_ref.py builds from the file; the temp file is gone.  The two files do not depend on the batch size, the merge window or
the number of logical devices; the flag alone writes no PREFIX.bam; two query files, an empty one, and the refused combinations."""
import glob
import gzip
import struct

import pytest

import bai_ref
import bam_ref
from test_gpu_cli_edit_distance import SAME, _run, _take

pytestmark = pytest.mark.gpu

SORTED = (".sorted.bam", ".sorted.bam.bai")
HD_SORTED = "@HD\tVN:1.6\tSO:coordinate\n"


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("bamsortcli")
    db = synth.make_db(str(d / "db"), n_genomes=4, genome_len=30_000, seed=11)
    rd = synth.make_reads(db, str(d / "r.fq"), n_reads=24, read_len=2000, seed=5)
    rd2 = synth.make_reads(db, str(d / "r2.fq"), n_reads=9, read_len=1500, seed=6)
    empty = str(d / "none.fq")
    open(empty, "wb").close()
    prefix, p2 = str(d / "out"), str(d / "second")
    base = ["mapDirectly", "--all", "-r", db.fasta, "-q", rd["path"], "-o", prefix]
    runs = {}
    for tag, args, env in (("bam", base + ["--bam"], None), ("both", base + ["--bam", "--bam-sorted"], None), ("alone", base + ["--bam-sorted"], None),
                           ("batch5", base + ["--bam-sorted"], {"MM_CLI_BATCH_READS": "5"}), ("batch7", base + ["--bam-sorted"], {"MM_CLI_BATCH_READS": "7"}),
                           ("window", base + ["--bam-sorted"], {"MM_CLI_BATCH_READS": "5", "MM_BAM_SORT_WINDOW_MB": "0"}),
                           ("two_devices", base + ["--bam-sorted", "--devices", "0,0"], {"MM_CLI_BATCH_READS": "5"}),
                           ("two_files", ["mapDirectly", "--all", "--bam", "--bam-sorted", "-r", db.fasta, "-q", rd["path"] + "," + rd2["path"], "-o", prefix + "," + p2], None),
                           ("empty", ["mapDirectly", "--all", "--bam", "--bam-sorted", "-r", db.fasta, "-q", empty, "-o", prefix], None)):
        p = _run(args, env)
        assert p.returncode == 0, (tag, p.stderr.decode()[-2000:])
        runs[tag] = _take(prefix)
        if tag == "two_files":
            runs["second"] = _take(p2)
    return dict(db=db, runs=runs, q=rd["path"], contigs=[(cid.split()[0], len(seq)) for cid, seq in zip(db.contig_ids, db.contig_seqs)])


def records(bam):
    """(header text, the records' bytes in file order) of a .bam"""
    raw = gzip.decompress(bam)
    _, at = bai_ref.header_end(raw)
    text, out = raw[8:8 + struct.unpack_from("<i", raw, 4)[0]].decode(), []
    while at < len(raw):
        size = 4 + struct.unpack_from("<i", raw, at)[0]
        out.append(raw[at:at + size])
        at += size
    return text, out


def check_sorted(world, run, unsorted_bam):
    """the two files of a run against the PREFIX.bam of the same mappings"""
    text, want = records(unsorted_bam)
    got_text, got = records(run[".sorted.bam"])
    assert got_text == text.replace(bam_ref.HD_LINE, HD_SORTED) and got_text.startswith(HD_SORTED) and "GO:" not in got_text
    assert got == sorted(want, key=lambda r: struct.unpack_from("<ii", r, 4))          # (sorted() is stable: ties stay in PREFIX.bam's order)
    assert bam_ref.decode(run[".sorted.bam"])[1] == world["contigs"]
    every = bam_ref.members(run[".sorted.bam"])
    ms = every[len(every) - 1 - -(-sum(len(r) for r in got) // 65280):]   # (the records' members and the end-of-file block: the header's come first)
    assert all(len(raw) == 65280 for _, raw in ms[:-2]) and ms[-1][0] == bam_ref.EOF_BLOCK
    assert run[".sorted.bam.bai"] == bai_ref.build(run[".sorted.bam"])
    assert ".sorted.bam.tmp" not in run
    return got


def test_sorted_beside_unsorted(world):
    a, b = world["runs"]["bam"], world["runs"]["both"]
    assert set(b) == set(a) | set(SORTED)
    for suf in a:                                                   # every other file of the run, PREFIX.bam among them, is what it was
        assert a[suf] == b[suf], suf
    got = check_sorted(world, b, a[".bam"])
    keys = [struct.unpack_from("<ii", r, 4) for r in got]
    assert len(got) >= 30 and len({k[0] for k in keys}) >= 3 and keys != [struct.unpack_from("<ii", r, 4) for r in records(a[".bam"])[1]]
    assert any(struct.unpack_from("<H", r, 18)[0] & 0x100 for r in got)                  # secondary records are there
    idx = bai_ref.parse(b[".sorted.bam.bai"])
    assert sum(x["pseudo"][1][0] for x in idx if x["pseudo"]) == len(got)


def test_the_flag_alone_writes_no_unsorted_file(world):
    a, b, c = world["runs"]["bam"], world["runs"]["both"], world["runs"]["alone"]
    assert set(c) == set(a) - {".bam"} | set(SORTED)
    for suf in c:
        assert c[suf] == b[suf], suf


@pytest.mark.parametrize("tag", ["batch5", "batch7", "window", "two_devices"])
def test_files_do_not_depend_on_batches_window_or_devices(world, tag):
    b, r = world["runs"]["both"], world["runs"][tag]
    for suf in SORTED + ("", ".editDistances"):
        assert r[suf] == b[suf], (tag, suf)
    assert ".sorted.bam.tmp" not in r


def test_two_query_files(world):
    first, second = world["runs"]["two_files"], world["runs"]["second"]
    for suf in SORTED + (".bam",):
        assert first[suf] == world["runs"]["both"][suf], suf
    got = check_sorted(world, second, second[".bam"])
    assert 3 <= len(got) != len(records(first[".bam"])[1])


def test_empty_input(world):
    run = world["runs"]["empty"]
    text, got = records(run[".sorted.bam"])
    assert got == [] and text.startswith(HD_SORTED) and run[".sorted.bam"].endswith(bam_ref.EOF_BLOCK) and len(bam_ref.members(run[".sorted.bam"])) == 2
    assert run[".sorted.bam.bai"] == bai_ref.build(run[".sorted.bam"]) == b"BAI\1" + struct.pack("<i", len(world["contigs"])) + struct.pack("<ii", 0, 0) * len(world["contigs"]) + bytes(8)
    assert ".sorted.bam.tmp" not in run


def test_refused_combinations(world, tmp_path):
    db, q, x = world["db"], world["q"], str(tmp_path / "x")
    maps = str(tmp_path / "m")
    open(maps, "wb").write(world["runs"]["bam"][""])
    for args in (["mapDirectly", "--bam-sorted", "--hpc", "-r", db.fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--bam-sorted", "--shard-index", "-r", db.fasta, "-q", q, "-o", x],
                 ["mapAgainstIndex", "--bam-sorted", "-i", x, "-q", q, "-o", x],
                 ["classify", "--bam-sorted", "--DB", db.dir, "--mappings", maps]):
        p = _run(args)
        assert p.returncode == 1 and "--bam-sorted" in p.stderr.decode(), (args, p.stderr.decode()[-500:])
        assert glob.glob(x + "*") == [] and glob.glob(maps + ".*") == [], args
