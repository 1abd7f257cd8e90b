// The devices of a run as the command line names them (--gpus N, --devices a,b,..), and the check every call of the C ABI goes through.
#pragma once
#include "../../../include/metamaps_hip.h"
#include "cli_common.hpp"
#include "host_util.hpp"

namespace {

void ck(mm_ctx* ctx, int st, const char* what) { if (st != MM_OK) die(std::string(what) + ": " + mm_last_error(ctx)); }

// one logical GPU: a context (stream + allocator) on a physical device, and the chunk indexes that live there
struct Dev { int phys = 0; mm_ctx* ctx = nullptr; std::vector<mm_index*> idx; };

void check_devices(const std::vector<int>& phys) {                // (the first HIP call of the process: the runtime comes up here)
  const int n = mm_device_count();
  if (n <= 0) die("No MI355X (gfx950) device available — this build has no CPU path");
  for (int p : phys) if (p < 0 || p >= n) die("device " + std::to_string(p) + " requested but only " + std::to_string(n) + " visible");
}

std::vector<int> device_list(const Options& o, bool check = true) {   // --gpus N: devices 0..N-1; --devices a,b,..: explicit (a device may repeat: test hook)
  std::vector<int> phys;
  if (o.v.count("devices")) for (auto& s : split(o.v.at("devices"), ",")) phys.push_back(std::stoi(s));
  else { const int g = o.v.count("gpus") ? std::stoi(o.v.at("gpus")) : 1; for (int i = 0; i < g; ++i) phys.push_back(i); }
  if (phys.empty()) die("--gpus must be at least 1");
  if (check) check_devices(phys);
  return phys;
}

}  // namespace
