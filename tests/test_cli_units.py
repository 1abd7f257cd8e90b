"""The command line program's device-free host code — CliSwitches (metamaps_amd/csrc/host/cli_switches.hpp) and the arithmetic of `classify`
(metamaps_amd/csrc/host/taxonomy.hpp) — compiled on its own with g++ under the address and undefined-behaviour sanitizers and run as a stand-alone
program (tests/test_cli_units.cpp): the switches' defaults and clamps, the taxonomy on a five-node tree, the coverage windows, how classify reads
a mapping quality, and the binomial tail against Boost.Math's answers (tests/golden/binom_golden.json).  CPU."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("cli_units") / "t")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", p, os.path.join(HERE, "test_cli_units.cpp"), "-lpthread"], check=True, timeout=600)
    return p


def test_switches_taxonomy_coverage_and_mapping_quality(exe, tmp_path):
    tax = tmp_path / "taxonomy"
    tax.mkdir()
    nodes = [("1", "1", "no rank", "root"), ("2", "1", "superkingdom", "Bacteria"), ("10", "2", "genus", "Escherichia"),
             ("100", "10", "species", "Escherichia coli"), ("x7", "100", "no rank", "Escherichia coli strain 7")]
    (tax / "nodes.dmp").write_text("".join(f"{i}\t|\t{p}\t|\t{r}\t|\t\t|\n" for i, p, r, _ in nodes))
    (tax / "names.dmp").write_text("".join(f"{i}\t|\t{n}\t|\t\t|\tscientific name\t|\n" for i, _, _, n in nodes) + "100\t|\tE. coli\t|\t\t|\tsynonym\t|\n")
    p = subprocess.run([exe, "self", str(tax)], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr).decode()[-3000:]
    assert p.stdout.decode().splitlines()[-1] == "ok"


def test_binomial_cdf_against_boost(exe):
    """The `sf` rows of the table are P(X > k): binomial_cdf is its complement, and the incomplete beta function it stands on is that tail itself,
    I_p(k + 1, n - k).  The tail is held to the tolerance tests/test_oracle_golden.py holds the oracle's to on the same rows (rel 1e-9); the
    cdf to the same relative tolerance against 1 - sf, or to the one rounding of that subtraction (an ulp of 1) where that is larger."""
    g = json.load(open(os.path.join(HERE, "golden", "binom_golden.json")))
    rows = [(n, p, k, v) for n, p, k, v in g["sf"] if 0 < p < 1 and 0 <= k < n]
    assert len(rows) > 50
    p = subprocess.run([exe, "binom"], input="".join(f"{n} {pp!r} {k}\n" for n, pp, k, _ in rows).encode(), capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    got = [tuple(map(float, ln.split())) for ln in p.stdout.decode().splitlines()]
    assert len(got) == len(rows)
    worst_tail = max(abs(t - v) / v for (_, t), (_, _, _, v) in zip(got, rows) if v > 0)
    print(f"binomial tail: worst relative error {worst_tail:.3g} over {len(rows)} rows")
    for (cdf, tail), (n, pp, k, v) in zip(got, rows):
        assert tail == pytest.approx(v, rel=1e-9, abs=1e-300), (n, pp, k)
        assert cdf == pytest.approx(1 - v, rel=1e-9, abs=2.3e-16), (n, pp, k)
