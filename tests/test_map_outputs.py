"""The text and byte rules of mapDirectly's side outputs — the lines of PREFIX.editDistances (metamaps_amd/csrc/host/edit_dist.hpp) and PREFIX.paf
(paf_out.hpp), the header, mapping qualities, flags and names of PREFIX.bam (bam_out.hpp) and the table of the side files (side_files.hpp) — compiled
on their own with g++ under the address and undefined-behaviour sanitizers and run as a stand-alone program (tests/test_map_outputs.cpp).  Every expected
value is stated here: literal strings, or tests/bam_ref.py's restatement of the BAM rules.  CPU."""
import os
import subprocess

import pytest

import bam_ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("map_outputs") / "t")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", p, os.path.join(HERE, "test_map_outputs.cpp"), "-lpthread"], check=True, timeout=600)
    return p


def run(exe, *args, rc=0):
    p = subprocess.run([exe, *args], capture_output=True, timeout=120)
    assert p.returncode == rc, (p.returncode, (p.stdout + p.stderr).decode(errors="replace")[-3000:])
    return p


def test_edit_distance_lines(exe):
    """two reads, three records, both strands; d = -1 prints NA NA NA"""
    assert run(exe, "edit").stdout == b"r1 cA + 3 10 58\nr1 cB - NA NA NA\nr2 cB - 0 99 148\n"


def test_paf_line(exe):
    """5= 1X 2I 3D 4=: 9 matches, block length 15, NM 6; last + 1 in column 9; the unaligned record before it has no line"""
    assert run(exe, "paf").stdout == b"q1\t12\t0\t12\t-\tctg\t5000\t100\t113\t9\t15\t255\tNM:i:6\tcg:Z:5=1X2I3D4=\n"


@pytest.mark.parametrize("contigs", [[("kraken:taxid|562|NC_000913.3", 4641652), ("c2", 7)], []], ids=["two_contigs", "no_contig"])
def test_bam_header(exe, contigs):
    assert run(exe, "header", *[str(x) for c in contigs for x in c]).stdout == bam_ref.header(contigs)


def test_mapq_from_the_text_of_field_14(exe):
    """bam_line_q reads the last field of every line (the last line has no newline), bam_mapq turns it into BAM's MAPQ"""
    texts = ["0", "-0", "1", "0.999999", "0.9999991", "0.99999", "0.9", "0.5", "1e-05", "1e-320"]
    want = [bam_ref.mapq_from_text(t) for t in texts]
    assert want == [0, 0, 60, 60, 60, 50, 10, 3, 0, 0]              # (the restatement itself, by hand: 1 - q <= 1e-6 is 60; -10 log10(1e-5) = 50)
    assert [int(x) for x in run(exe, "mapq", *texts).stdout.split()] == want


def test_flag_primary_record_and_names(exe):
    """read 0 ("aa"): three aligned records of equal q, the first is primary.  read 1 ("bbb"): its largest q belongs to an unaligned record, so the
    largest aligned one (0.7, strand -) is primary.  Lines: read strand contig flag mapq name_end; then name_off[0] and the joined names."""
    out = run(exe, "fields", "R", "2", "0.5,3,1", "0.5,4,-1", "0.5,0,1", "R", "3", "0.9,-1,1", "0.2,5,1", "0.7,2,-1").stdout.decode().splitlines()
    q = bam_ref.mapq_from_text
    assert out == [f"0 1 0 0 {q('0.5')} 2", f"0 -1 1 {0x10 | 0x100} {q('0.5')} 4", f"0 1 2 {0x100} {q('0.5')} 6",
                   f"1 1 0 {0x100} {q('0.9')} 9", f"1 1 1 {0x100} {q('0.2')} 12", f"1 -1 2 {0x10} {q('0.7')} 15", "0 aaaaaabbbbbbbbb"]


def test_name_length_matters_only_for_reads_with_a_record(exe):
    out = run(exe, "fields", "R", "300", "0.4,-1,1").stdout.decode().splitlines()   # no aligned record: no BAM record will carry the name
    assert out == [f"0 1 0 {0x100} {bam_ref.mapq_from_text('0.4')} 300", "0 " + "a" * 300]
    assert run(exe, "fields", "R", "254", "0.4,3,1").stdout.decode().splitlines()[0] == f"0 1 0 0 {bam_ref.mapq_from_text('0.4')} 254"


def test_a_255_byte_name_with_an_aligned_record_ends_the_program(exe):
    p = run(exe, "fields", "R", "255", "0.4,3,1", rc=1)
    assert b"--bam" in p.stderr and b"254" in p.stderr and p.stdout == b""


@pytest.mark.parametrize("flags, want", [(["edit-distance"], [".editDistances"]), (["paf"], [".editDistances", ".paf"]), (["bam"], [".editDistances", ".bam bgzf"]),
                                         (["paf", "bam"], [".editDistances", ".paf", ".bam bgzf"]), ([], [])],
                         ids=["edit_distance", "paf", "bam", "paf_bam", "none"])
def test_side_file_table(exe, flags, want):
    assert run(exe, "table", *flags).stdout.decode().splitlines() == want


def test_bgzf_end_of_file_block(exe):
    assert run(exe, "eof").stdout == bam_ref.EOF_BLOCK
