"""The host code stays readable: no function of metamaps_amd/csrc/host/ or of the library's host code (metamaps_amd/csrc/*.hip) above 200 lines (round-4 review: map_mode was
one 797-line function, classify_one 280; round 6: map_batch 997), and none of the device allocator (mm_alloc.hpp and the two headers beside it) above 60; no file of
metamaps_amd/csrc/host/ above 800 lines (the CLI was one file of 2 488; map_run.hpp later stood at 999 by squeezing its lines) and no line of them above 200 characters.  CPU."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_function_above_200_lines_in_the_host_program():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "func_lengths.py")], capture_output=True, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    longest = int(out.split()[0])
    assert 40 < longest <= 200, out                                # (40 <: the script did find the functions)
    counts = out.strip().split("\n")[-1].split()                   # "functions: N csrc/host M csrc/*.hip A csrc/mm_alloc.hpp+..."
    assert counts[0] == "functions:" and int(counts[3]) >= 30, out # (the library's .hip files were parsed)
    assert counts[6].startswith("csrc/mm_alloc.hpp") and int(counts[5]) >= 15, out   # (the device allocator's headers were parsed; the script holds their functions to 60 lines)
    files = out.strip().split("\n")[-2].split()                    # "longest file: L csrc/host/NAME of N csrc/host"
    assert files[:2] == ["longest", "file:"] and int(files[5]) >= 14, out   # (the CLI's headers were counted)
    assert 200 < int(files[2]) <= 800, out
    wide = out.strip().split("\n")[-3].split()                     # "longest line: W csrc/host/NAME:LINE"
    assert wide[:2] == ["longest", "line:"] and 100 < int(wide[2]) <= 200, out   # (100 <: the lines were measured)
    assert not any("load_reference" in ln for ln in out.split("\n")[:12]), out     # (once the longest host function of the CLI, 137 lines: now ref_loader.hpp's pieces)
    parsed = out.strip().split("\n")[-4].split()                   # "library files: NAME.hip ..."
    assert parsed[:2] == ["library", "files:"] and "mm_merge.hip" in parsed and "mm_api.hip" in parsed, out   # (the chunk merge is library host code under the 200-line rule)


HOST = os.path.join(ROOT, "metamaps_amd", "csrc", "host")


def host_sources():
    return {n: open(os.path.join(HOST, n)).read() for n in sorted(os.listdir(HOST)) if n.endswith((".hpp", ".cpp"))}


def test_the_run_outputs_are_declared_once():
    """What the command line asks mapDirectly to write is parsed and combined in output_plan.hpp alone: main and MapRun name no output's option struct and no flag
    helper, nobody writes an implied --edit-distance back into the options, the precedence of the flag a refusal names and the decimal validator stand in one
    file each, and map_run.hpp is shorter than the 796 lines it had when every new output took a line of it."""
    src = host_sources()
    for name in ("map_run.hpp", "metamaps_main.cpp"):
        code = re.sub(r"//[^\n]*", "", src[name])
        for ident in ("PileupOpts", "VcfOpts", "ConsOpts", "ModsOpts", "MotifOpts", "DepthOpts", "errprof_of", "errprof_or", "modflag", "bam_sorted_of"):
            assert not re.search(r"\b" + ident + r"\b", code), (name, ident)
    assert not [n for n, s in src.items() if 'o.v["edit-distance"] =' in s]
    assert [n for n, s in src.items() if '"--consensus" :' in s] == ["output_plan.hpp"]
    assert [n for n, s in src.items() if "const bool decimal" in s] == ["cli_common.hpp"]
    assert 200 < src["map_run.hpp"].count("\n") < 796
    plan = src["output_plan.hpp"]                                  # device-free: none of the headers that name a call of the C ABI, directly
    assert not re.search(r'#include "(bam_sort_out|batch_outputs|run_outputs|cli_device|bam_out|paf_out|edit_dist)\.hpp"', plan) and "metamaps_hip.h" not in plan


def test_classify_is_split_by_stage_and_its_first_half_is_device_free():
    """classify_run.hpp (788 lines, one struct of 35 members, when this was written) keeps the run and its device calls; the lines, the tables, the EM driver and
    the writers have a header each, the first two without the C ABI (tests/test_mapping_lines.cpp compiles them alone); the formatter of the mapping lines and a
    batch's outputs take LineMeta and KeptLines without the rest of classify; cleanF stands once, and so does the length of a line's read ID."""
    src = host_sources()
    new = ("mapping_lines.hpp", "classify_tables.hpp", "em_sharded.hpp", "classify_outputs.hpp")
    assert 100 < src["classify_run.hpp"].count("\n") <= 450
    for name in new:
        assert 20 < src[name].count("\n") <= 400, name
    for name in ("mapping_lines.hpp", "classify_tables.hpp"):
        assert "metamaps_hip.h" not in src[name] and not re.search(r'#include "(cli_device|em_sharded|classify_run)\.hpp"', src[name]), name
    assert re.findall(r'#include "([^"]+)"', src["mapping_lines.hpp"]) == ["cli_common.hpp"]
    for name in ("map_format.hpp", "batch_outputs.hpp"):
        assert '#include "classify_run.hpp"' not in src[name] and '#include "mapping_lines.hpp"' in src[name], name
    assert [n for n, s in src.items() if "const double minF" in s] == ["taxonomy.hpp"]
    assert not [n for n, s in src.items() if "memchr(B.p, ' '" in s or "memchr(A.p, ' '" in s]
    assert [n for n, s in src.items() if "struct ClassifyOpts" in s] == ["cli_common.hpp"]
    assert [n for n, s in src.items() if re.search(r"\bClassifyOpts classify_options\(.*\) \{", s)] == ["metamaps_main.cpp"]
    assert [n for n, s in src.items() if 'o.v.at("minreads")' in s] == ["metamaps_main.cpp"] and src["metamaps_main.cpp"].count('o.v.at("minreads")') == 1


def test_the_c_surface_holds_no_kernels_no_rccl_and_no_stand_in_declarations():
    """mm_api.hip turns exceptions into status codes and owns handle lifetimes: device code and collectives live in the units it calls, and what
    it calls is declared in their headers, where the compiler checks the declarations against the definitions."""
    src = open(os.path.join(ROOT, "metamaps_amd", "csrc", "mm_api.hip")).read()
    assert "__global__" not in src and "<<<" not in src
    assert "rccl" not in src and "nccl" not in src
    assert "namespace mm {" not in src
    mk = open(os.path.join(ROOT, "metamaps_amd", "csrc", "Makefile")).read()
    assert "mm_merge.hip" in mk
