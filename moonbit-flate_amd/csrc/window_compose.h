// window_compose.h -- the operator of flate_hip_inflate_one's COMPOSE step, written ONCE: plain C++17 without HIP,
// compiled into the kernels (one_kernels.hip, one_probe_kernel.inc) and into tests/host_model/window_compose_model.cpp.
//
// A unit's TAIL FUNCTION T is its final 32 KiB window as a function of the 32 KiB window W in front of the unit: 32768
// entries of 16 bits, entry j for the byte 32768 - j places in front of the unit's end.  An entry is a LITERAL byte
// (0 .. 255) or, with kWinRef set, "byte (entry & 0x7fff) of W".  A unit shorter than 32 KiB passes the rest of W
// through, shifted.  Composition is associative -- (A o B) o C == A o (B o C), both "apply C, then B, then A" -- so the
// windows in front of all units of a round come from one scan.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define WC_HD __host__ __device__ inline
#else
#define WC_HD inline
#endif

namespace flate {

constexpr uint32_t kWinEntries = 32768;
constexpr uint16_t kWinRef = 0x8000;

// the identity's entry j: byte j of the window in front
WC_HD uint16_t wc_identity(uint32_t j) { return (uint16_t)(kWinRef | j); }
// entry `outer` of a later function over the earlier function `inner` (kWinEntries entries): outer o inner
WC_HD uint16_t wc_compose(uint16_t outer, const uint16_t *inner) {
  return (outer & kWinRef) ? inner[outer & 0x7fffu] : outer;
}
// the entry as a byte, given the resolved window in front (kWinEntries bytes; bytes in front of the stream are 0)
WC_HD uint8_t wc_resolve(uint16_t e, const uint8_t *prev) { return (e & kWinRef) ? prev[e & 0x7fffu] : (uint8_t)e; }

}  // namespace flate
