// splice_rule.h -- where the pieces of spliced DEFLATE streams lie, written ONCE: plain C++17 without HIP, compiled
// into the kernels (splice_kernels.hip), into the library's host code (api_checks.h, flate_api_deflate.hip) and into
// tests/host_model/splice_rule_model.cpp, which compares it with a Python walk over bit positions.  grouped_place at
// the end is the specification of group_scan_kernel: the kernel must equal it on every input.
//
// A piece without stored blocks just adds its bit count: f(x) = x + a.  A stored block pads to a byte boundary of the
// stream (write_stored_header -> flush, huffman-bit-writer.mbt:474-487,139-158), so a piece with one maps the position
// as f(x) = align8(x + a) + b: a = bits in front of the first stored block + its 3 header bits, b = everything after
// that boundary (itself independent of x).  These maps are closed under composition:
//   (a1,-) then (a2,-)   = (a1+a2, -)          (a1,-)  then (a2,b2) = (a1+a2, b2)
//   (a1,b1) then (a2,-)  = (a1, b1+a2)         (a1,b1) then (a2,b2) = (a1, align8(b1+a2) + b2)
//
// GROUPS.  Several spliced streams in one output, each inside a container: behind the last piece of a group come the
// closing block of Writer::close (3 bits, padding to a byte, LEN, NLEN), the container's trailer and the next group's
// header -- x -> align8(x + 3) + 32 + 8 * (trailer + next header), one more map of the same form.  Members start on
// bytes, so a position counted from out[0] is congruent mod 8 to the position inside the member's own stream, and the
// padding of stored blocks comes out the same in both.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SPLICE_HD __host__ __device__ inline
#else
#define SPLICE_HD inline
#endif

namespace flate {

constexpr uint64_t kNoStored = ~0ull;

struct PosMap {
  uint64_t a, b;  // b == kNoStored: x -> x + a; else x -> align8(x + a) + b
};
SPLICE_HD uint64_t align8(uint64_t x) { return (x + 7) & ~7ull; }
SPLICE_HD uint64_t apply(const PosMap &f, uint64_t x) { return f.b == kNoStored ? x + f.a : align8(x + f.a) + f.b; }
SPLICE_HD PosMap then(const PosMap &f, const PosMap &g) {  // first f, then g
  PosMap r;
  if (f.b == kNoStored) {
    r.a = f.a + g.a;
    r.b = g.b;
  } else {
    r.a = f.a;
    r.b = g.b == kNoStored ? f.b + g.a : align8(f.b + g.a) + g.b;
  }
  return r;
}

// The end of a group: closing block, trailer, the next group's header (0 behind the last group).
SPLICE_HD PosMap group_close_map(uint32_t trailer_len, uint32_t next_header_len) {
  return PosMap{3, 32 + 8 * ((uint64_t)trailer_len + next_header_len)};
}
// header_len (per group) or, where that is null, the same length for every group
SPLICE_HD uint32_t group_header_len(const uint32_t *header_len, uint32_t header_len_all, uint32_t g) {
  return header_len ? header_len[g] : header_len_all;
}

// The groups of a call: group g is the pieces [group_off[g], group_off[g + 1]), at least one each (an empty stream is
// one piece of zero bytes, whose wavefront writes the closing block).
inline bool grouped_args_ok(const uint32_t *group_off, uint32_t n_groups, uint32_t n_pieces) {
  if (!group_off || group_off[0] != 0 || group_off[n_groups] != n_pieces) return false;
  for (uint32_t g = 0; g < n_groups; ++g)
    if (group_off[g + 1] <= group_off[g]) return false;
  return true;
}

// The serial walk.  sum: the pieces' maps {a, b}, two words each.  piece_bit[i]: the absolute bit, counted from
// out[0], of piece i's first block; end_bit[g]: where group g's last piece ends (its closing block starts);
// payload_off[g]: the first byte of group g's raw stream; member_off[g]: that minus the header, member_off[n_groups]
// and the return value: the total.
inline uint64_t grouped_place(const uint64_t *sum, uint32_t n_pieces, const uint32_t *group_off, uint32_t n_groups,
                              const uint32_t *header_len, uint32_t header_len_all, uint32_t trailer_len,
                              uint64_t *piece_bit, uint64_t *end_bit, uint64_t *payload_off, uint64_t *member_off) {
  (void)n_pieces;
  uint64_t x = n_groups ? 8ull * group_header_len(header_len, header_len_all, 0) : 0ull;
  for (uint32_t g = 0; g < n_groups; ++g) {
    payload_off[g] = x >> 3;
    member_off[g] = (x >> 3) - group_header_len(header_len, header_len_all, g);
    for (uint32_t i = group_off[g]; i < group_off[g + 1]; ++i) {
      piece_bit[i] = x;
      x = apply(PosMap{sum[2 * (uint64_t)i], sum[2 * (uint64_t)i + 1]}, x);
    }
    end_bit[g] = x;
    const uint32_t next = g + 1 < n_groups ? group_header_len(header_len, header_len_all, g + 1) : 0u;
    x = apply(group_close_map(trailer_len, next), x);
  }
  member_off[n_groups] = x >> 3;
  return x >> 3;
}

// flate_hip_zip_write with the option "zip_piece_bytes" = P >= 1: an entry longer than P bytes is ceil(len / P)
// pieces of P bytes, the last one shorter; every other entry is one piece.  Two passes over the entries, O(pieces):
// the count (and how many entries are long), then the pieces' in_off (count + 1 entries) and group_off (n + 1).
inline uint64_t zip_pieces_count(const uint64_t *in_off, uint32_t n, uint64_t P, uint32_t *long_entries) {
  uint64_t pieces = 0;
  uint32_t longs = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t len = in_off[i + 1] - in_off[i];
    if (P >= 1 && len > P) {
      pieces += len / P + (len % P ? 1u : 0u);
      ++longs;
    } else {
      pieces += 1;
    }
  }
  if (long_entries) *long_entries = longs;
  return pieces;
}
// (the caller has counted: at most 2^32 - 2 pieces)
inline void zip_pieces_plan(const uint64_t *in_off, uint32_t n, uint64_t P, uint64_t *piece_in_off, uint32_t *group_off) {
  uint32_t k = 0;
  for (uint32_t i = 0; i < n; ++i) {
    group_off[i] = k;
    const uint64_t lo = in_off[i], hi = in_off[i + 1];
    if (P >= 1 && hi - lo > P) {
      for (uint64_t at = lo; at < hi; at += P) piece_in_off[k++] = at;
    } else {
      piece_in_off[k++] = lo;
    }
  }
  group_off[n] = k;
  piece_in_off[k] = in_off[n];
}

}  // namespace flate
