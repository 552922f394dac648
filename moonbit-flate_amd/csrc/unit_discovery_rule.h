// unit_discovery_rule.h -- the arithmetic of the unit discoveries and of the readers' window carry, written ONCE: plain
// C++17 without HIP, compiled into the library's host code (unit_discovery.h, unit_rounds.h) and into
// tests/host_model/unit_discovery_rule_model.cpp.
#pragma once

#include <stdint.h>

namespace flate {

// the nodes a chain's arrays hold at most (chain_size refuses more: path_len is a power of two >= cap + 2)
constexpr uint32_t kChainCapMax = 0x7ffffff0u;

// THE SIZE RULE of a chain over two lists: List A's na candidates and List B's nb nodes fit one chain -- *cap = their
// sum -- or they do not (the counts saturate at 2^32 - 1, so the sum is taken in 64 bits).
inline bool two_list_cap(uint32_t na, uint32_t nb, uint32_t *cap) {
  if ((uint64_t)na + nb > kChainCapMax) return false;
  *cap = na + nb;
  return true;
}

// THE CARRY's index: the units of the last of the rounds that go over n_dec units (>= 1) per_round (>= 1) at a time.
// The round driver leaves the window behind unit i of a round in R[i + 1], so R[unit_last_count] is the window behind
// the call's last unit.
inline uint32_t unit_last_count(uint32_t n_dec, uint32_t per_round) {
  return n_dec - ((n_dec - 1u) / per_round) * per_round;
}

}  // namespace flate
