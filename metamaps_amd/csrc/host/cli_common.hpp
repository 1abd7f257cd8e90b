// What every part of the command line program stands on: the two ways out (die, finish_fast), the phase clock, thread helpers and the parsed
// command line.  The standard library only: taxonomy.hpp and the CPU tests include this without the device's C ABI.
#pragma once
#include <sys/stat.h>
#include <unistd.h>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace {

// MM_CLI_TIMING=1: wall time per phase on stderr at exit
struct PhaseClock {
  const bool timing;
  explicit PhaseClock(bool timing_) : timing(timing_) {}
  std::map<std::string, double> acc; std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now(), t0 = t; std::mutex m;
  void add(const char* name, double seconds) { std::lock_guard<std::mutex> lk(m); acc[name] += seconds; }   // worker threads: summed over the workers
  void lap(const char* name) { auto n = std::chrono::steady_clock::now(); add(name, std::chrono::duration<double>(n - t).count()); t = n;
                               if (timing) std::cerr << "INFO, lap " << name << " at +" << std::chrono::duration<double>(n - t0).count() << " s\n"; }
  bool reported = false;
  void report() { if (reported) return; reported = true; if (timing) for (auto& kv : acc) std::cerr << "INFO, time " << kv.first << " " << kv.second << " s\n"; }
  ~PhaseClock() { report(); }
};

// Every output file is written and closed: leave without the orderly teardown.  Returning 150 GB of index to the driver allocation by
// allocation (hipFree) took 2.5 s of a 13 s run at miniSeq+H scale; the operating system reclaims the process' device memory as a
// whole.  (MM_CLI_FULL_TEARDOWN=1 keeps the orderly path: the tests of handle lifetimes under a leak checker use it.)
[[noreturn]] void finish_fast() { std::cout.flush(); std::cerr.flush(); fflush(nullptr); _exit(0); }

// An error exit leaves through _exit: helper threads (the HIP runtime coming up beside the parse of `classify`, the worker contexts' prewarm, the
// readers) may be inside the driver at this moment, and exit() would run static destructors and the runtime's atexit handlers under them.
[[noreturn]] void die(const std::string& m) { std::cerr << m << std::endl; std::cout.flush(); fflush(nullptr); _exit(1); }
// a helper thread that is joined on every way out of its scope (an exception that passes a joinable std::thread ends in std::terminate)
struct JoinOnExit { std::thread& t; ~JoinOnExit() { if (t.joinable()) t.join(); } };

template <typename F> void on_each(size_t n, F&& fn) {           // fn(i) for i < n, concurrently
  if (n == 1) { fn(0); return; }
  std::vector<std::thread> th;
  for (size_t i = 0; i < n; ++i) th.emplace_back([&fn, i] { fn(i); });
  for (auto& t : th) t.join();
}

// the same with fn(0) on the calling thread, which goes on with whatever fn(0) does behind its share while the others run
template <typename F> void on_each_caller_first(size_t n, F&& fn) {
  std::vector<std::thread> th;
  for (size_t i = 1; i < n; ++i) th.emplace_back([&fn, i] { fn(i); });
  fn(0);
  for (auto& t : th) t.join();
}

uint64_t file_size(const std::string& f) {                       // commonFunc.hpp:211-231
  struct stat st; if (stat(f.c_str(), &st) != 0) die("Cannot open " + f + " for size determination.");
  return (uint64_t)st.st_size;
}

// the command line as parse() of metamaps_main.cpp leaves it: option values by their long names, the plain flags
struct Options { std::map<std::string, std::string> v; bool all = false, stream = false, shard = false, em_host = false; };
// The two shapes an option's number takes, for every *_options parser: whether the value is well-formed, and the value.  The ranges and the messages are the callers'.
// Digits alone, 1 to max_digits of them (strtoull: past 64 bits it saturates and sets errno to ERANGE, which only --bootstrap-seed's 20 digits can reach).
struct IntegerValue { bool ok; unsigned long long value; };
inline IntegerValue integer_value(const std::string& v, size_t max_digits) {
  const bool digits = !v.empty() && v.size() <= max_digits && v.find_first_not_of("0123456789") == std::string::npos;
  return {digits, digits ? strtoull(v.c_str(), nullptr, 10) : 0};
}
// Digits with at most one point and at least one digit (1, 0.25, .5, 1.), 32 bytes at most: no sign, no exponent
struct DecimalValue { bool ok; double value; };
inline DecimalValue decimal_value(const std::string& v) {
  const bool decimal = !v.empty() && v.size() <= 32 && v.find_first_not_of("0123456789.") == std::string::npos && v.find_first_of("0123456789") != std::string::npos &&
                       v.find('.') == v.rfind('.');
  return {decimal, decimal ? strtod(v.c_str(), nullptr) : 0};
}
// --bootstrap B [--bootstrap-seed S] (classify, mapDirectly --then-classify; not in the reference): B read-level Poisson bootstrap replicates of
// the EM after the point estimate, PREFIX.EM.WIMP.bootstrap beside the WIMP.  B = 0: off (nothing changes, no file appears).
struct BootOpts { int B = 0; uint64_t seed = 1; };
// --lca T (classify, mapDirectly --then-classify; not in the reference): the confidence threshold of the LCA assignment, a decimal in [0.51, 1].
// Off without the flag: nothing changes and no file appears.
struct LcaOpts { bool on = false; double tau = 0; };
// --genes (classify, mapDirectly --then-classify; the reference's geneLevelAnalysis.pl): the gene- and annotation-level analysis of the reads' best
// mappings against DB/DB_annotations.txt and DB/DB_proteins.faa.annotated.  Off without the flag: nothing changes and no file appears.
struct GeneOpts { bool on = false; };
// --base-qualities, --min-base-quality Q (mapDirectly; not in the reference): the run keeps the queries' base qualities beside the bases on the device.
// --bam writes them into QUAL; Q (0..93, implies --base-qualities) is the floor below which --pileup, --vcf and --consensus do not count a base's evidence
// (mm_pileup_events_q).  Off without the flags: nothing changes.
struct QualOpts { bool keep = false; int min_base_quality = 0; };
// --min-identity T [--refit] (classify, mapDirectly --then-classify; the reference's util/filterLowIdentityEntities.pl): genomes whose best mappings have
// a median identity below T (a decimal in [0, 1], the script's --identityThreshold) are removed and their reads set to unclassified in PREFIX.EM-filtered*;
// --refit (not in the reference) also runs the EM again without the removed genomes' mappings.  Off without the flag: nothing changes and no file appears.
struct IdentOpts { bool on = false, refit = false; double T = 0; };
// What `classify` and `mapDirectly --then-classify` take from the command line beside the files; --minreads N: the reads a taxon needs to serve as the
// reference distribution of PREFIX.EM.evidenceUnknownSpecies (parseCmdArgs.hpp:462-471)
struct ClassifyOpts { BootOpts boot; LcaOpts lca; GeneOpts genes; IdentOpts ident; size_t minReadsU = 10000; };
ClassifyOpts classify_options(const Options& o, const std::string& mode);   // (metamaps_main.cpp: it ends the program on a malformed value or a flag outside its sub-commands)

}  // namespace
