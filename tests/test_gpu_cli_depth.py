"""`mapDirectly --depth`: PREFIX.depth.bedgraph, .depth.windows and .depth.contigs beside outputs that stay byte for byte, on the synthetic reference of the
other side-output tests with query files that span several batches.  The three files equal what tests/depth_ref.py computes from the intervals rebuilt from the
same run's PREFIX and PREFIX.editDistances (a read's primary record is its aligned line with the largest field 14, the first of equals); they agree with
PREFIX.pileup and .pileup.contigs of the same run and with --consensus' called positions; the same files come from two logical devices and from other batch
sizes; an empty run writes the empty files and the header; --compress-output leaves them plain; the refused combinations name the flag."""
import glob

import pytest

import depth_ref
from test_gpu_cli_edit_distance import SAME, _run, _take

pytestmark = pytest.mark.gpu
OURS = (".depth.bedgraph", ".depth.windows", ".depth.contigs")
BATCH = {"MM_CLI_BATCH_READS": "40"}
DEFAULT_T = (1, 5, 10, 30)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("depthcli")
    db = synth.make_db(str(d / "db"), n_genomes=4, genome_len=30_000, seed=11, contigs_per_genome=2, with_oddities=False)
    rd = synth.make_reads(db, str(d / "r.fq"), n_reads=150, read_len=2000, seed=5)
    even = [c for g in range(0, len(db.genome_contigs), 2) for c in db.genome_contigs[g]]
    cname, clen = [db.contig_ids[c].split()[0] for c in even], [len(db.contig_seqs[c]) for c in even]
    fasta = str(d / "even.fa")
    with open(fasta, "wb") as f:
        for c in even:
            f.write(b">" + db.contig_ids[c].encode() + b"\n" + db.contig_seqs[c].tobytes() + b"\n")
    prefix = str(d / "out")
    base = ["mapDirectly", "-r", fasta, "-q", rd["path"], "-o", prefix]
    cons = ["--consensus", "--consensus-min-depth", "3"]
    pile = ["--pileup", "--pileup-min-count", "1", "--pileup-min-frac", "0", "--all"]
    runs = {}
    for tag, extra, env in (("pileup_all", pile, BATCH), ("depth_pileup_all", ["--depth"] + pile, BATCH), ("depth", ["--depth"], BATCH),
                            ("plain", ["--edit-distance"], BATCH), ("two", ["--depth", "--devices", "0,0"], {"MM_CLI_BATCH_READS": "5"}),
                            ("batch7", ["--depth"], {"MM_CLI_BATCH_READS": "7"}), ("cons", cons, BATCH), ("depth_cons", ["--depth", "--depth-thresholds", "3"] + cons, BATCH),
                            ("options", ["--depth", "--depth-window", "700", "--depth-thresholds", "2,4"], BATCH), ("empty", ["--depth", "-m", "5000"], BATCH),
                            ("compress", ["--depth", "--compress-output"], BATCH)):
        p = _run(base + extra, env)
        assert p.returncode == 0, (tag, p.stderr.decode()[-2000:])
        runs[tag] = _take(prefix)
    return dict(db=db, cname=cname, clen=clen, runs=runs, fasta=fasta, q=rd["path"])


def _intervals(world, run):
    """the (contig, first, last) of every read's primary aligned record, from the run's own PREFIX and PREFIX.editDistances"""
    maps, eds = run[""].decode().splitlines(), run[".editDistances"].decode().splitlines()
    assert len(maps) == len(eds)
    best = {}
    for m, e in zip(maps, eds):
        f, g = m.split(" "), e.split(" ")
        assert f[0] == g[0]
        if g[3] == "NA":
            continue
        if f[0] not in best or float(f[13]) > best[f[0]][0]:       # the first of equals stays
            best[f[0]] = (float(f[13]), (world["cname"].index(f[5]), int(g[4]), int(g[5])))
    return [iv for _, iv in best.values()]


def _same_numbers(got, want, floats):
    g, w = got.decode().splitlines(), want.splitlines()
    assert len(g) == len(w)
    for a, b in zip(g, w):
        ca, cb = a.split("\t"), b.split("\t")
        assert len(ca) == len(cb), (a, b)
        for k, (x, y) in enumerate(zip(ca, cb)):
            if k in floats and not a.startswith("#"):
                assert abs(float(x) - float(y)) <= floats[k] * 1.0000001, (a, b)
            else:
                assert x == y, (a, b)


def _check_against_ref(world, run, window, thresholds):
    iv = _intervals(world, run)
    res = depth_ref.profile(world["clen"], iv, window, thresholds)
    assert run[".depth.bedgraph"].decode() == depth_ref.bedgraph_text(res, world["cname"])
    _same_numbers(run[".depth.windows"], depth_ref.windows_text(res, world["cname"], world["clen"], window), {5: 1e-3})
    _same_numbers(run[".depth.contigs"], depth_ref.contigs_text(res, world["cname"], world["clen"], thresholds), {5: 1e-3, 8: 1e-6, 9: 1e-6})
    return iv, res


def test_the_three_files_equal_the_restatement(world):
    iv, res = _check_against_ref(world, world["runs"]["depth"], 1000, DEFAULT_T)
    assert len(iv) >= 50 and len(res["contig"]) >= 2 and len(res["runs"]) > 100 and max(r[3] for r in res["runs"]) >= 3   # the world is not degenerate
    assert world["runs"]["depth"][".depth.contigs"].decode().splitlines()[0] == depth_ref.contigs_header(DEFAULT_T)[:-1]
    _check_against_ref(world, world["runs"]["options"], 700, (2, 4))
    _check_against_ref(world, world["runs"]["depth_pileup_all"], 1000, DEFAULT_T)   # under --all a read with several records counts once


def test_depth_beside_the_pileup(world):
    a, b = world["runs"]["pileup_all"], world["runs"]["depth_pileup_all"]
    assert set(b) == set(a) | set(OURS)
    for suf in a:                                                   # every shared file is byte-identical
        assert a[suf] == b[suf], suf
    ours = [ln.split("\t") for ln in b[".depth.contigs"].decode().splitlines()[1:]]
    theirs = [ln.split("\t") for ln in b[".pileup.contigs"].decode().splitlines()]
    assert [c[:5] for c in ours] == theirs and len(theirs) >= 2     # contigID length alignments covered sumDepth
    runs = {}
    for ln in b[".depth.bedgraph"].decode().splitlines():
        c = ln.split("\t")
        runs.setdefault(c[0], []).append((int(c[1]), int(c[2]), int(c[3])))
    sites = b[".pileup"].decode().splitlines()
    assert len(sites) > 20
    for ln in sites:                                                # every site's depth is the bedgraph's depth at its position
        c = ln.split("\t")
        hit = [d for s, e, d in runs[c[0]] if s <= int(c[1]) < e]
        assert hit == [int(c[5])], ln


def test_depth_alone_changes_no_other_file(world):
    a, b = world["runs"]["plain"], world["runs"]["depth"]
    assert set(b) == set(a) | set(OURS)
    for suf in SAME + (".editDistances",):
        assert a[suf] == b[suf], suf


@pytest.mark.parametrize("tag", ["two", "batch7", "depth_pileup_all"])
def test_the_same_files_from_other_devices_and_batches(world, tag):
    a, b = world["runs"]["depth"], world["runs"][tag]
    for suf in OURS:
        assert b[suf] == a[suf], (tag, suf)


def test_ge3_is_the_consensus_called_column(world):
    a, b = world["runs"]["cons"], world["runs"]["depth_cons"]
    assert set(b) == set(a) | set(OURS)
    for suf in a:
        assert a[suf] == b[suf], suf
    called = {ln.split("\t")[0]: ln.split("\t")[3] for ln in b[".consensus.tsv"].decode().splitlines()[1:]}
    lines = b[".depth.contigs"].decode().splitlines()
    assert lines[0].split("\t")[-1] == "ge3" and len(lines[0].split("\t")) == 11
    assert {ln.split("\t")[0]: ln.split("\t")[-1] for ln in lines[1:]} == called and len(called) >= 2 and any(int(v) > 0 for v in called.values())


def test_an_empty_run_writes_the_empty_files_and_the_header(world):
    run = world["runs"]["empty"]                                    # no read is as long as -m asks
    assert run[".depth.bedgraph"] == b"" and run[".depth.windows"] == b"" and run[".depth.contigs"].decode() == depth_ref.contigs_header(DEFAULT_T) and run.get("", b"") == b""


def test_compress_output_leaves_the_three_files_plain(world):
    a, b = world["runs"]["depth"], world["runs"]["compress"]
    assert ".gz" in b
    for suf in OURS:
        assert b[suf] == a[suf], suf


def test_refused_combinations(world, tmp_path):
    db, q, fasta, x = world["db"], world["q"], world["fasta"], str(tmp_path / "x")
    maps = str(tmp_path / "m")
    open(maps, "wb").write(world["runs"]["plain"][""])
    io = ["-r", fasta, "-q", q, "-o", x]
    for args in (["mapDirectly", "--depth", "--hpc"] + io,
                 ["mapDirectly", "--depth", "--shard-index"] + io,
                 ["mapDirectly", "--depth", "--pileup", "--vcf", "--hpc"] + io,
                 ["mapAgainstIndex", "--depth", "-i", x, "-q", q, "-o", x],
                 ["classify", "--depth", "--DB", db.dir, "--mappings", maps],
                 ["mapDirectly", "--depth-window", "500"] + io,
                 ["mapDirectly", "--pileup", "--depth-thresholds", "1,2"] + io,
                 ["mapDirectly", "--depth", "--depth-window", "0"] + io,
                 ["mapDirectly", "--depth", "--depth-thresholds", "5,5"] + io,
                 ["mapDirectly", "--depth", "--depth-thresholds", "10,5"] + io,
                 ["mapDirectly", "--depth", "--depth-thresholds", "1,2,3,4,5,6,7,8,9"] + io):
        p = _run(args)
        assert p.returncode == 1 and "--depth" in p.stderr.decode(), (args, p.stderr.decode()[-500:])
        assert glob.glob(x + "*") == [] and glob.glob(maps + ".*") == [], args
