// Read-level Poisson bootstrap of the EM: the weight w(r, i) that replicate r gives read i ("Bootstrap").
// A counter-based draw, never stored: x = mix(seed ^ mix(r << 32 | i)), u = x >> 11 (53 bits), w = #{k : T_k <= u} with
// T_k = floor(2^53 * P(Poisson(1) <= k)), k = 0..15.  Integer arithmetic only, so host, device and a numpy restatement agree bit for bit.
//
// Compiles for host (unit tests: tests/test_boot_core.cpp via g++) and device.
#pragma once
#include <stdint.h>

#ifndef MM_HD
#if defined(__HIPCC__)
#define MM_HD __host__ __device__ inline
#else
#define MM_HD inline
#endif
#endif

namespace mm {

// splitmix64's finaliser
MM_HD uint64_t boot_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

constexpr int BOOT_MAX_WEIGHT = 16;

// w = number of thresholds <= u.  The thresholds as immediates (a table in memory would be a lookup per read on the device): the first
// one decides 37 % of the draws, the second another 37 %.
MM_HD int boot_weight_of(uint64_t u) {
  int w = 0;
  w += u >= 3313563428353947ull; w += u >= 6627126856707895ull; w += u >= 8283908570884869ull; w += u >= 8836169142277194ull;
  w += u >= 8974234285125275ull; w += u >= 9001847313694891ull; w += u >= 9006449485123161ull; w += u >= 9007106938184342ull;
  w += u >= 9007189119816990ull; w += u >= 9007198251109506ull; w += u >= 9007199164238758ull; w += u >= 9007199247250508ull;
  w += u >= 9007199254168154ull; w += u >= 9007199254700280ull; w += u >= 9007199254738289ull; w += u >= 9007199254740823ull;
  return w;
}

// weight of read i (0-based among the reads with at least one mapping) in replicate r
MM_HD int boot_weight(uint64_t seed, uint32_t r, uint32_t i) {
  const uint64_t x = boot_mix(seed ^ boot_mix(((uint64_t)r << 32) | (uint64_t)i));
  return boot_weight_of(x >> 11);
}

}  // namespace mm
