// carve.h -- one device buffer carved into a call's arrays (host only; plain C++17 without HIP, so that
// tests/host_model/chain_walk_model.cpp compiles it too).
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace flate_host {

// One buffer carved into a call's arrays, every one on a 256-byte boundary, in the order of the take() calls.  The
// same lines run twice: over a null base for the size (`at` when they are through), then over the buffer.  slack: bytes
// behind the count entries that still belong to the array.
struct Carve {
  void *base = nullptr;
  size_t at = 0;
  template <typename T>
  void take(T *&p, size_t count, size_t slack = 0) {
    p = (T *)((uintptr_t)base + at);
    at += (count * sizeof(T) + slack + 255) & ~(size_t)255;
  }
};

}  // namespace flate_host
