"""metamaps_amd/csrc/mm_prims.hpp's with_scratch — the one place that runs rocprim's "null pointer = tell me the size" protocol — on a host
build with a stub buffer and fake calls (tests/test_with_scratch.cpp): a call that reports 0 bytes still gets a non-null buffer of at least
16 bytes, the buffer grows to what a call reports and is never shrunk, the size query and the real call happen exactly once each, an empty
buffer is refused before the real call, and errors of either call come out.  CPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_with_scratch_never_hands_a_null_buffer_to_the_real_call(tmp_path):
    exe = str(tmp_path / "tscratch")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "test_with_scratch.cpp")], check=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("ok "), (out + p.stderr.decode())[-500:]
    assert int(out.split()[1]) >= 40, out
