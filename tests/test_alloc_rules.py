"""metamaps_amd/csrc/mm_alloc_rules.hpp (the device allocator's sizing rules: rounding, cache fit, headroom, index-scale size classes, the pool's
one-eighth rule — arithmetic only, no device) against their formulas restated in tests/test_alloc_rules.cpp: powers of two +-1 from 1 byte to 256 GiB
and 100 000 random sizes; at most 12.5 % slack for cached blocks, at most 1.6 % and a 16 MiB granule for index-scale classes, monotone.  CPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_sizing_rules_match_their_formulas_and_bounds(tmp_path):
    exe = str(tmp_path / "talloc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "test_alloc_rules.cpp")], check=True, timeout=300)
    p = subprocess.run([exe, "100000"], capture_output=True, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("ok "), out[-500:]
    assert int(out.split()[1]) >= 100000 + 3 * 39 - 1, out
