"""bench.py plumbing that runs without a GPU: the database directory written around device-generated contigs for the CPU baseline /
CLI sample must be one the reference's `classify` accepts (here: the oracle CLI, end to end, with -t N)."""
import json
import os
import subprocess

import numpy as np


def test_sample_db_dir_runs_through_oracle_map_and_classify(oracle_lib, tmp_path):
    import orc
    from metamaps_amd import synth
    rng = np.random.default_rng(4)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genomes = [rng.choice(acgt, size=40_000) for _ in range(5)]
    genomes[3][2000:2600] = ord("N")
    db = synth.write_db_dir(str(tmp_path / "db"), [(7 + 3000 * i, g.tobytes()) for i, g in enumerate(genomes)] + [(7, rng.choice(acgt, size=9_000).tobytes())])
    fq = str(tmp_path / "r.fq")
    with open(fq, "wb") as f:
        for r in range(60):
            g = genomes[r % 5]; p = int(rng.integers(0, 40_000 - 3000)); s = g[p:p + 3000].copy()
            m = rng.random(3000) < 0.05; s[m] = rng.choice(acgt, size=int(m.sum()))
            f.write(f"@r{r}\n".encode() + s.tobytes() + b"\n+\n" + b"I" * 3000 + b"\n")
    out = {}
    for t in ("1", "4"):
        pre = str(tmp_path / f"o{t}")
        p = subprocess.run([orc.CLI, "mapDirectly", "--all", "-r", db["fasta"], "-q", fq, "-o", pre, "-w", "8", "-t", t], capture_output=True, check=True, timeout=600)
        js = json.loads(p.stderr.decode().strip().splitlines()[-1])
        assert js["reads"] == 60 and js["mappings"] >= 50
        subprocess.run([orc.CLI, "classify", "--DB", db["dir"], "--mappings", pre, "-t", t], capture_output=True, check=True, timeout=600)
        out[t] = (open(pre).read(), open(pre + ".EM.WIMP").read(), open(pre + ".EM.reads2Taxon").read())
    assert out["1"] == out["4"]                                   # the threaded index build / mapping of the oracle change nothing
    assert "1000007" in out["1"][2] and os.path.exists(str(tmp_path / "o1.EM.evidenceUnknownSpecies"))


def test_bench_arguments_parse():
    import sys
    import bench
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1"]
        a = bench.parse_args()
    finally:
        sys.argv = argv
    assert a.shape == "community" and a.reads == 100_000 and a.read_len == 10_000 and a.window == 8


def _parse(*extra):
    import sys
    import bench
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1"] + list(extra)
        return bench.parse_args()
    finally:
        sys.argv = argv


def test_bench_steps_and_dump_arguments():
    import pytest
    a = _parse("--steps", "5", "--warmup", "0", "--dump-outputs", "d")
    assert a.steps == 5 and a.warmup == 0 and a.dump_outputs == "d"
    for bad in (("--steps", "0"), ("--config", "3", "--dump-outputs", "d")):
        with pytest.raises(SystemExit):
            _parse(*bad)


def test_bench_side_measurements_need_full():
    """a plain run measures the headline alone: --full is off by default, and a side measurement asked for without it is refused"""
    import pytest
    assert not _parse().full and _parse("--full").full
    assert _parse("--full", "--measure-free-overlap").measure_free_overlap
    with pytest.raises(SystemExit):
        _parse("--measure-free-overlap")


def test_step_outputs_and_dump_within_budget(tmp_path, monkeypatch):
    """what a step returns, as float64 arrays; all of it when it fits, else the same seeded rows of the large arrays, under the budget"""
    import bench
    from metamaps_amd import capi
    rng = np.random.default_rng(1)
    rec = np.zeros(5000, dtype=capi.RECORD_DTYPE)
    rec["ref_contig"] = rng.integers(0, 2**31 - 1, len(rec)); rec["mapq"] = rng.random(len(rec))
    off = np.linspace(0, len(rec), 1001).astype(np.int64)
    out = bench.step_outputs(off, rec, rng.random(30), rng.random(7), rng.random(len(rec)), rng.integers(0, len(rec), 1000))
    assert all(a.dtype == np.float64 and a.ndim == 1 for a in out.values())
    assert np.array_equal(out["mapping_ref_contig"], rec["ref_contig"]) and np.array_equal(out["mapping_offsets"], off)

    assert bench.dump_outputs(str(tmp_path / "all"), out) == 1.0
    for n, a in out.items():
        assert np.array_equal(np.load(str(tmp_path / "all" / (n + ".npy"))), a)

    monkeypatch.setattr(bench, "DUMP_BYTES", 120_000)              # a budget the records do not fit: scaled down
    monkeypatch.setattr(bench, "DUMP_WHOLE_BYTES", 1_000)
    d1, d2 = tmp_path / "s1", tmp_path / "s2"
    frac = bench.dump_outputs(str(d1), out)
    assert 0.0 < frac < 1.0 and bench.dump_outputs(str(d2), out) == frac
    assert sum(p.stat().st_size for p in d1.iterdir()) <= 120_000
    for n, a in out.items():
        got = np.load(str(d1 / (n + ".npy")))
        assert np.array_equal(got, np.load(str(d2 / (n + ".npy"))))
        if a.nbytes > 1_000:
            rows = np.load(str(d1 / (n + ".rows.npy"))).astype(np.int64)
            assert np.array_equal(got, a[rows]) and len(rows) == int(a.size * frac)
        else:
            assert np.array_equal(got, a) and not (d1 / (n + ".rows.npy")).exists()
