"""metamaps_amd/csrc/mm_size_classes.hpp (which instance of the K2 / K4 LDS radix sort a read takes — arithmetic only, no device) against the
rule restated in tests/test_size_classes.cpp: for every count from 0 to 20 000, and around every power of two up to 2^64, the class is the
smallest listed IPT with 256 * IPT >= count; no minimizer, and zero or one hit, need no sort; counts beyond the last class go to the
segmented sort.  CPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_size_classes_match_the_rule_for_every_count(tmp_path):
    exe = str(tmp_path / "tcls")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "test_size_classes.cpp")], check=True, timeout=300)
    p = subprocess.run([exe, "20000"], capture_output=True, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("ok "), out[-500:]
    assert int(out.split()[1]) >= 20001, out
