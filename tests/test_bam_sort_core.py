"""The sorter's definitions (metamaps_amd/csrc/mm_bam_sort_core.hpp: the order's key, the window's pieces and the copy of bytes at any residues, the
virtual offsets, the chunk rule, the linear rule, the .bai's bytes), built for the host with g++ — plain, and as a stand-alone program under the address and
undefined-behaviour sanitizers — and run through the steps of the device's merge (tests/test_bam_sort_core.cpp) on the record sets of
tests/bam_sort_cases.py: the gathered stream is the records in the defined order at every window size, and the index is tests/bai_ref.py's, byte for
byte.  CPU."""
import os
import subprocess

import pytest

import bai_ref
import bam_ref
import bam_sort_cases
import bam_writer

HERE = os.path.dirname(os.path.abspath(__file__))
MEMBER = bam_sort_cases.MEMBER
CASES = {"edges": bam_sort_cases.edges, "ties": bam_sort_cases.ties, "one_run": bam_sort_cases.one_run, "nothing": bam_sort_cases.nothing}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("bam_sort_core") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_bam_sort_core.cpp")], check=True, timeout=300)
    return p


@pytest.fixture(scope="module")
def files():
    """per case: (the case, the sorted stream, a .bam of it with zlib's members of 65 280 bytes, the header members' bytes): made once, never changed"""
    out = {}
    for name, make in CASES.items():
        case = make()
        stream = b"".join(bam_sort_cases.sorted_stream(case))
        head = bam_writer.bgzf_block(bam_sort_cases.header(case["ref_len"]))
        body = [bam_writer.bgzf_block(stream[a:a + MEMBER], 1) for a in range(0, len(stream), MEMBER)]
        out[name] = (case, stream, head + b"".join(body) + bam_ref.EOF_BLOCK, len(head), [len(m) for m in body])
    return out


def run(exe, case, header_bytes, window, member_sizes):
    lines = [f"{len(case['ref_len'])} {header_bytes} {window} {len(case['runs'])}"]
    for records in case["runs"]:
        raw = b"".join(records)
        lines.append(str(len(records)) + "".join(f" {r} {b} {e} {s}" for r, b, e, s in bam_sort_cases.coords(raw)))
        lines.append(raw.hex() or "-")
    lines.append(" ".join(str(x) for x in [len(member_sizes)] + member_sizes))
    p = subprocess.run([exe], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
    stream, bai = p.stdout.decode().split()
    return (b"" if stream == "-" else bytes.fromhex(stream)), bytes.fromhex(bai)


@pytest.mark.parametrize("name", sorted(CASES))
def test_stream_and_index(exe, files, name):
    case, stream, bam, header_bytes, member_sizes = files[name]
    want_bai = bai_ref.build(bam, bam_sort_cases.coords)
    for window in (MEMBER, 2 * MEMBER, 4096 * MEMBER):
        got, bai = run(exe, case, header_bytes, window, member_sizes)
        assert got == stream, window
        assert bai == want_bai, window


def test_the_index_answers_regions(exe, files):
    """the index the header's steps made, read back and asked: what query() names holds every record that overlaps"""
    case, _, bam, header_bytes, member_sizes = files["edges"]
    _, recs = bai_ref.placed(bam, bam_sort_cases.coords)
    idx = bai_ref.parse(run(exe, case, header_bytes, 2 * MEMBER, member_sizes)[1])
    assert [len(x["ioff"]) for x in idx] == [1, 0, 1 << 15, 0, 1 + ((max(e for r, _, e, _, _ in recs if r == 4) - 1) >> 14)]
    assert idx[1] == idx[3] == dict(bins={}, pseudo=None, ioff=[]) and idx[2]["pseudo"][1] == (18, 0)
    for ref, beg, end in bam_sort_cases.regions(case):
        chunks = bai_ref.query(idx, ref, beg, end)
        got = [k for k, (r, b, e, vs, ve) in enumerate(recs) if any(a <= vs < z for a, z in chunks) and r == ref and b < end and e > beg]
        assert got == [k for k, (r, b, e, vs, ve) in enumerate(recs) if r == ref and b < end and e > beg], (ref, beg, end)
