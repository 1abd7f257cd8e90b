// The text files of a stored index (`metamaps index` writes them, `metamaps mapAgainstIndex` reads them back; mapWrap.h:358-405, :443-554):
//   PREFIX.index       0 while the index is being written; then 1 and the chunk files, one per line
//   PREFIX.arguments   the parameters the index was built with, "key value" per line
//   PREFIX.contigs     contig ID, length and chunk number (from 1) of every contig, tab-separated, in the reference's order
// The chunk files themselves (PREFIX.N.seqset, or .N.mmidx with --full-index) are the library's: MapRun stores and loads them.  No device call here.
#pragma once
#include "cli_common.hpp"
#include "host_util.hpp"
#include <fstream>

namespace {

struct IndexChunk { int first, count; std::string file; };       // contigs [first, first + count) of the reference; file: where a stored chunk lies

// the parameters that travel with an index
struct IndexArguments {
  int k = 16, w = 0, minLen = 1000;
  float pi = 80;
  double pval = 1e-3;
  uint64_t refSize = 0, maxMem = 0;
  std::string ref;
};

void write_index_flag(const std::string& ipre, int done, const std::vector<std::string>& chunk_files) {   // mapWrap.h:363-366, :395-402
  std::ofstream flag(ipre + ".index");
  if (!flag.is_open()) die("Cannot open " + ipre + ".index");
  flag << done << "\n";
  for (auto& fn : chunk_files) { flag << fn << "\n"; std::cout << "Stored state in file " << fn << "\n"; }
}
void write_index_arguments(const std::string& ipre, const IndexArguments& a) {
  std::ofstream args(ipre + ".arguments");
  if (!args.is_open()) die("Cannot open file " + ipre + ".arguments for serialization.");
  args.precision(17);
  args << "kmerSize " << a.k << "\nwindowSize " << a.w << "\nminReadLength " << a.minLen << "\npercentageIdentity " << a.pi << "\np_value " << a.pval
       << "\nreferenceSize " << a.refSize << "\nmaximumMemory " << a.maxMem << "\nreference " << a.ref << "\n";
}
void write_index_contigs(const std::string& ipre, const std::vector<IndexChunk>& chunks, const std::vector<std::string>& cname, const std::vector<int>& clen) {
  std::ofstream cf(ipre + ".contigs");
  for (size_t c = 0; c < chunks.size(); ++c)
    for (int i = chunks[c].first; i < chunks[c].first + chunks[c].count; ++i) cf << cname[(size_t)i] << "\t" << clen[(size_t)i] << "\t" << c + 1 << "\n";
}

IndexArguments read_index_arguments(const std::string& ipre) {    // mapWrap.h:447-461
  std::ifstream a(ipre + ".arguments");
  if (!a.is_open()) die("Cannot open file " + ipre + ".arguments for deserialization.");
  std::string key, val; std::map<std::string, std::string> kv;
  while (a >> key && std::getline(a, val)) { while (!val.empty() && val[0] == ' ') val.erase(0, 1); kv[key] = val; }
  for (const char* need : {"kmerSize", "windowSize", "minReadLength", "percentageIdentity", "p_value", "referenceSize", "maximumMemory", "reference"})
    if (!kv.count(need)) die("Index " + ipre + " is incomplete (" + need + " missing in .arguments)");
  IndexArguments r;
  r.k = std::stoi(kv["kmerSize"]); r.w = std::stoi(kv["windowSize"]); r.minLen = std::stoi(kv["minReadLength"]); r.pi = std::stof(kv["percentageIdentity"]);
  r.pval = std::stod(kv["p_value"]); r.refSize = std::stoull(kv["referenceSize"]); r.maxMem = std::stoull(kv["maximumMemory"]); r.ref = kv["reference"];
  return r;
}
// the chunk list and the contig table of a stored index: contigs appended to cname / clen, their bases added to ref_bases
void read_index_files(const std::string& ipre, std::vector<std::string>& cname, std::vector<int>& clen, uint64_t& ref_bases, std::vector<IndexChunk>& chunks) {
  std::ifstream flag(ipre + ".index");
  if (!flag.is_open()) die("Index " + ipre + " not found (" + ipre + ".index)");
  int done = 0; flag >> done;
  if (done != 1) die("Index " + ipre + " is not complete.");    // mapWrap.h:466-470
  std::vector<std::string> chunk_files; std::string fn;
  while (flag >> fn) chunk_files.push_back(fn);
  std::ifstream cf(ipre + ".contigs");
  if (!cf.is_open()) die("Cannot open " + ipre + ".contigs");
  std::vector<int> chunk_of; std::string line;
  while (std::getline(cf, line)) {
    auto fl = split(line, "\t");
    if (fl.size() != 3) die("Weird line in " + ipre + ".contigs");
    cname.push_back(fl[0]); clen.push_back(std::stoi(fl[1])); chunk_of.push_back(std::stoi(fl[2])); ref_bases += (uint64_t)clen.back();
  }
  for (size_t c = 0; c < chunk_files.size(); ++c) {
    int first = -1, count = 0;
    for (size_t i = 0; i < chunk_of.size(); ++i) if (chunk_of[i] == (int)c + 1) { if (first < 0) first = (int)i; ++count; }
    chunks.push_back(IndexChunk{first < 0 ? 0 : first, count, chunk_files[c]});
  }
}

}  // namespace
