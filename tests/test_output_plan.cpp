// CPU unit test of OutputPlan (metamaps_amd/csrc/host/output_plan.hpp): what a mapDirectly command line asks for, and the questions the run asks about the
// combination.  That header alone is included, so it compiles without the device's C ABI.  For every subset of the twelve flags below (bit i of the mask is flag
// i; --mod-motifs only beside --mods, without which it is refused) one line:
//   MASK edit flag_name traceback reads_until_text keep_reads intervals per_file_state vcf_table SIDESET
// with the predicates as 0 / 1, flag_name as - where no refusal can be made (edit is 0) and the SideSet as N_SIDE characters 0 / 1.  The expected lines are the Python side's (tests/test_output_plan.py).
// Built and run by tests/test_output_plan.py with g++, plain and with -fsanitize=address,undefined (no GPU needed).
#include "../metamaps_amd/csrc/host/output_plan.hpp"
#include <cstdio>

int main() {
  static const char* const flag[12] = {"edit-distance", "paf", "bam", "bam-sorted", "pileup", "vcf", "consensus", "mods", "mod-motifs", "depth", "error-profile", "extract-unmapped"};
  for (unsigned mask = 0; mask < (1u << 12); ++mask) {
    if ((mask >> 8 & 1u) && !(mask >> 7 & 1u)) continue;
    Options o;
    for (int i = 0; i < 12; ++i) if (mask >> i & 1u) o.v[flag[i]] = i == 7 ? "C+m" : i == 8 ? "CG:0" : "1";
    const OutputPlan p = output_plan(o, "mapDirectly");
    std::string side;
    for (int s = 0; s < N_SIDE; ++s) side += p.side[(size_t)s] ? '1' : '0';
    printf("%u %d %s %d %d %d %d %d %d %s\n", mask, (int)p.edit(), p.edit() ? p.flag_name() : "-", (int)p.traceback(), (int)p.reads_until_text(), (int)p.keep_reads(), (int)p.intervals(),
           (int)p.per_file_state(), (int)p.vcf_table(), side.c_str());
  }
  return 0;
}
