"""`classify` and `mapDirectly --then-classify` after the split of classify_run.hpp by stage write what the commit before the split wrote: every .EM* file (and
PREFIX.extractedIdentities) byte for byte and the same stdout, the one timing figure of the bootstrap line masked, on a 10-genome annotated database with 200 reads:
plain; --bootstrap 8 --lca 0.8 --genes --min-identity 0.9 --refit together; a BGZF mappings file; MM_CLASSIFY_THREADS=64; two EM ranks with --em-host-reduce
(--gpus 2 where two devices are visible, else --devices 0,0: two ranks on the one device, the same code); mapDirectly --then-classify.

The other side is the `metamaps` program of commit PARENT, built once from `git archive` of its csrc/ against this tree's library (the split touches no .hip file and
not the C ABI).  Where that is not possible (no git history, or a later ABI the old sources do not compile against) it is tests/golden/classify_parent.json: per run
the SHA-256 and size of every file and the masked stdout, recorded from that same program by `python tests/test_gpu_classify_parity.py PARENT_BINARY OUT.json` on
a GPU.  Equal digests are equal bytes."""
import glob
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "metamaps_amd", "csrc")
CLI = os.path.join(CSRC, "metamaps")
PARENT = "7d8c06c640cdce2d3e594cc7b5fecc1970d0e52a"
GOLDEN = os.path.join(HERE, "golden", "classify_parent.json")
ALL_FLAGS = ["--bootstrap", "8", "--lca", "0.8", "--genes", "--min-identity", "0.9", "--refit"]

pytestmark = pytest.mark.gpu


def two_ranks():
    import torch
    return (["--gpus", "2"] if torch.cuda.device_count() >= 2 else ["--devices", "0,0"]) + ["--em-host-reduce"]


def make_world(d):
    """The database, the reads and their mappings (plain and BGZF), made with this tree's program: both sides classify the same bytes."""
    import gene_db
    from metamaps_amd import synth
    db = gene_db.make(os.path.join(d, "db"), n_genomes=10, genome_len=30_000, seed=7)
    rd = synth.make_reads(db, os.path.join(d, "r.fq"), n_reads=200, read_len=3000, seed=3, abundance_sigma=0.5)
    w = {"dir": d, "db": db, "q": rd["path"], "m": os.path.join(d, "map0"), "mz": os.path.join(d, "mapz")}
    subprocess.run([CLI, "mapDirectly", "--all", "-r", db.fasta, "-q", rd["path"], "-o", w["m"]], check=True, capture_output=True, timeout=300)
    subprocess.run([CLI, "mapDirectly", "--all", "--compress-output", "-r", db.fasta, "-q", rd["path"], "-o", w["mz"]], check=True, capture_output=True, timeout=300)
    assert os.path.getsize(w["m"]) > 10_000
    return w


def run_all(exe, w, side):
    """The six runs with the program `exe`, each on a prefix of its own under DIR/side: {run: {"stdout": masked text, suffix: [sha256, size]}}."""
    out_dir = os.path.join(w["dir"], side)
    os.mkdir(out_dir)
    classify = ["classify", "--DB", w["db"].dir, "--minreads", "3", "--mappings"]
    runs = {"plain": ("m", [], {}), "all_flags": ("m", ALL_FLAGS, {}), "bgzf": ("mz", [], {}), "threads64": ("m", [], {"MM_CLASSIFY_THREADS": "64"}),
            "two_ranks": ("m", two_ranks(), {}), "then_classify": (None, [], {})}
    got = {}
    for tag, (src, extra, env) in runs.items():
        pre = os.path.join(out_dir, tag)
        if src is None:
            args = ["mapDirectly", "--all", "-r", w["db"].fasta, "-q", w["q"], "-o", pre, "--then-classify", w["db"].dir, "--minreads", "3"]
        else:
            for f in glob.glob(w[src] + "*"):
                shutil.copy(f, pre + f[len(w[src]):])
            args = classify + [pre] + extra
        p = subprocess.run([exe] + args, capture_output=True, timeout=300, env=dict(os.environ, **env))
        assert p.returncode == 0, (side, tag, p.stderr.decode()[-2000:])
        text = p.stdout.decode().replace(out_dir, "@OUT").replace(w["dir"], "@DIR")
        got[tag] = {"stdout": re.sub(r"(EM iterations per replicate, )\S+( s on )", r"\1T\2", text)}
        for f in sorted(glob.glob(pre + ".EM*") + glob.glob(pre + ".extractedIdentities")):
            b = open(f, "rb").read()
            got[tag][f[len(pre):]] = [hashlib.sha256(b).hexdigest(), len(b)]
        assert ".EM.WIMP" in got[tag] and got[tag][".EM"][1] > 10_000, (side, tag)
    assert ".EM.WIMP.bootstrap" in got["all_flags"] and ".EM-filtered.refit.WIMP" in got["all_flags"] and ".EM.geneLevelAnalysis" in got["all_flags"]
    assert "Bootstrap: 8 replicates" in got["all_flags"]["stdout"] and ", T s on " in got["all_flags"]["stdout"]
    return got


def build_parent(d):
    """The parent commit's `metamaps` from its sources, or None."""
    try:
        src = os.path.join(d, "parent_src")
        os.mkdir(src)
        subprocess.run(["git", "-C", ROOT, "cat-file", "-e", PARENT + "^{commit}"], check=True, capture_output=True, timeout=60)
        tar = subprocess.run(["git", "-C", ROOT, "archive", PARENT, "metamaps_amd/csrc", "include"], check=True, capture_output=True, timeout=120).stdout
        subprocess.run(["tar", "-x", "-C", src], input=tar, check=True, timeout=120)
        exe = os.path.join(d, "metamaps_parent")
        subprocess.run(["g++", "-O3", "-std=c++17", "-o", exe, os.path.join(src, "metamaps_amd", "csrc", "host", "metamaps_main.cpp"), "-L" + CSRC, "-lmetamaps_hip", "-lz",
                        "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, timeout=600)
        return exe
    except (subprocess.CalledProcessError, subprocess.TimeoutExpired, OSError):
        return None


@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("classify_parity"))
    w = make_world(d)
    exe = build_parent(d)
    parent = run_all(exe, w, "parent") if exe else json.load(open(GOLDEN))["runs"]
    if not exe:                                                    # the recorded side classified these very bytes
        want = json.load(open(GOLDEN))["mappings_sha256"]
        assert hashlib.sha256(open(w["m"], "rb").read()).hexdigest() == want, "the mappings differ from those tests/golden/classify_parent.json was recorded on"
    return {"parent": parent, "this": run_all(CLI, w, "this")}


@pytest.mark.parametrize("tag", ["plain", "all_flags", "bgzf", "threads64", "two_ranks", "then_classify"])
def test_classify_writes_what_the_parent_commit_wrote(sides, tag):
    a, b = sides["parent"][tag], sides["this"][tag]
    assert sorted(a) == sorted(b)
    for suf in sorted(a):
        if suf != "stdout":
            assert list(a[suf]) == list(b[suf]), suf
    assert a["stdout"] == b["stdout"]


if __name__ == "__main__":                                         # record the golden side: PARENT_BINARY OUT.json
    import tempfile
    sys.path.insert(0, ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        world = make_world(tmp)
        rec = {"parent": PARENT, "mappings_sha256": hashlib.sha256(open(world["m"], "rb").read()).hexdigest(), "runs": run_all(os.path.abspath(sys.argv[1]), world, "parent")}
    json.dump(rec, open(sys.argv[2], "w"), indent=1, sort_keys=True)
