"""OutputPlan (metamaps_amd/csrc/host/output_plan.hpp): what a mapDirectly command line asks for and the questions the run asks about the combination,
for every subset of the twelve output flags.  tests/test_output_plan.cpp includes that header alone (so it needs nothing of the device's C ABI), is built with
g++ plain and under the address and undefined-behaviour sanitizers and run as a stand-alone program.  The expected lines are restated here from the code the
plan replaced, each rule where it stood: main's implication of --edit-distance and its precedence of the flag a refusal names, side_files_of, the two
conditions of BatchSideOutputs::from_mapping (traceback; reads released), the condition of from_text's accumulators and RunVariants::resize.  CPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["edit-distance", "paf", "bam", "bam-sorted", "pileup", "vcf", "consensus", "mods", "mod-motifs", "depth", "error-profile", "extract-unmapped"]
SIDE_ROWS = ["edit-distance", "paf", "bam", "extract-unmapped", "extract-mapped", "extract-taxa", "deplete-taxa"]   # the rows of side_files.hpp, the first three aligned


def restated(given):
    """One subset as the code before the plan treated it."""
    f = set(given)
    # main: "all nine imply it and inherit its refusals"
    if f & {"paf", "bam", "bam-sorted", "pileup", "vcf", "consensus", "mods", "depth", "error-profile"}:
        f.add("edit-distance")
    edit = "edit-distance" in f
    # main and decide_placement: the flag a refusal is reported under
    name = "-"
    if edit:
        for flag in ("error-profile", "depth", "mods", "consensus", "vcf", "pileup", "bam", "bam-sorted", "paf", "edit-distance"):
            if flag in f:
                name = "--" + ("mod-motifs" if flag == "mods" and "mod-motifs" in f else flag)
                break
    # side_files_of, on the options main left
    side = [row in f for row in SIDE_ROWS]
    if any(side[:3]) or "bam-sorted" in f:
        side[0] = True
    # RunVariants::resize and the pointers MapRun made of it
    pile, vcf, mods, depth, errprof, srt = "pileup" in f, "vcf" in f or "consensus" in f, "mods" in f, "depth" in f, "error-profile" in f, "bam-sorted" in f
    extract = any(side[3:])
    traceback = side[1] or side[2] or srt or pile or vcf or mods or errprof               # from_mapping: mm_mapping_align, else the distances alone
    reads_until_text = side[2] or srt or pile or vcf or mods or depth or errprof or extract   # from_mapping: the negation resets the reads
    keep_reads = edit or extract                                                         # MapRun::keep_reads
    intervals = pile or vcf or depth                                                     # from_text: iv->add_intervals
    per_file_state = pile or vcf or mods or depth or errprof                             # resize: files.resize(n_files); from_text: the block of the accumulators
    cols = [edit, name, traceback, reads_until_text, keep_reads, intervals, per_file_state, vcf]
    return " ".join(c if isinstance(c, str) else str(int(c)) for c in cols) + " " + "".join(str(int(s)) for s in side)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("output_plan_" + request.param) / "t")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", *extra, "-o", p, os.path.join(HERE, "test_output_plan.cpp"), "-lpthread", "-lz"],
                   check=True, timeout=600)
    return p


def test_every_subset_of_the_output_flags(exe):
    p = subprocess.run([exe], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr).decode()[-3000:]
    got = p.stdout.decode().splitlines()
    want = []
    for mask in range(1 << len(FLAGS)):
        given = [FLAGS[i] for i in range(len(FLAGS)) if mask >> i & 1]
        if "mod-motifs" in given and "mods" not in given:          # refused: --mod-motifs needs --mods
            continue
        want.append(f"{mask} {restated(given)}")
    assert len(want) == 3 * (1 << 10)
    assert got == want
    # the restatement itself, by hand, at three corners
    assert want[0] == "0 0 - 0 0 0 0 0 0 0000000"
    assert f"{1 << 9} 1 --depth 0 1 1 1 1 0 1000000" in want       # --depth alone: no traceback, the reads kept to from_text
    assert f"{1 << 11} 0 - 0 1 1 0 0 0 0001000" in want            # --extract-unmapped alone: no alignment at all
