// gzfile_rule.h -- how the units of a gzip FILE chain across its members (flate_hip_gzfile_index / _read), written
// ONCE: plain C++17 without HIP, compiled into the kernels (gzfile_kernels.hip), into the library's host code and
// into tests/host_model/gzfile_rule_model.cpp, which compares it with the walk of tests/gzfile_ref.py.  The link kernel
// takes THE HOP through gzfile_parts_rule.h: the whole file is the part that is final, and gzfile_parts_hop(.., true)
// equals gzfile_hop in all three fields (tests/host_model/gzfile_parts_serial_rule_model.cpp sweeps it).
//
// Inside a member the units chain as the units of one stream do (deflate_block_rule.h): a unit that stops in front of
// a dynamic block header is followed by the unit that starts at that bit.  A unit that ends with BFINAL ends its
// member, and THE HOP says what follows: the member's trailer, then the file's end, or the next member's header and,
// behind it, the first unit of that member -- whatever block type is there.  Bits are counted from the FILE's first
// byte.  The header rule is gzip_rule.h's over in[e, in_len): a member's range is never clipped.
#pragma once

#include <stdint.h>

#include "gzip_rule.h"

namespace flate {

constexpr uint32_t kGzHopEnd = 0;   // the member ends where the file does: the terminal node
constexpr uint32_t kGzHopDead = 1;  // no member can start behind the trailer: FLATE_HIP_E_CORRUPT at `e`
constexpr uint32_t kGzHopNext = 2;  // the next member starts at byte e, its first unit at bit `bit`

struct GzHop {
  uint32_t kind;
  uint64_t e;    // where the member ends: the byte behind its trailer
  uint64_t bit;  // kGzHopNext: 8 * (e + the next header's length)
};

// where the member whose header starts at byte p has its first unit, or 0: no member can start at p (p < in_len)
GZIP_HD uint64_t gzfile_first_bit(const uint8_t *in, uint64_t in_len, uint64_t p) {
  const uint64_t hl = gzip_header_len(in + p, in_len - p);
  return hl ? 8u * (p + hl) : 0ull;
}

// THE HOP behind a final block that ends at bit b (b <= 8 * (in_len - 8): the decoders read nothing behind that)
GZIP_HD GzHop gzfile_hop(const uint8_t *in, uint64_t in_len, uint64_t b) {
  GzHop h;
  h.e = (b + 7u) / 8u + kGzipTrailerLen;
  h.bit = 0;
  if (h.e >= in_len) {
    h.kind = h.e == in_len ? kGzHopEnd : kGzHopDead;
    return h;
  }
  h.bit = gzfile_first_bit(in, in_len, h.e);
  h.kind = h.bit ? kGzHopNext : kGzHopDead;
  return h;
}

}  // namespace flate
