// bgzf_rule.h -- what a BGZF member is (SAM/BAM specification section 4.1: a gzip member, RFC 1952, whose extra field
// carries its own size), written ONCE: plain C++17 without HIP, compiled into the discovery kernels
// (bgzf_kernels.hip), into the library's host code and into tests/host_model/bgzf_index_model.cpp, which compares it
// with the serial walk of tests/bgzf_ref.py.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BGZF_HD __host__ __device__ inline
#else
#define BGZF_HD inline
#endif

namespace flate {

constexpr uint32_t kBgzfHeaderLen = 18;   // as this library and htslib write it: 12 + XLEN (6)
constexpr uint32_t kBgzfTrailerLen = 8;   // CRC-32, ISIZE
constexpr uint32_t kBgzfEofLen = 28;      // the canonical empty member that ends a file
constexpr uint32_t kBgzfMemberMax = 65536;  // BSIZE is 16 bits wide and holds the size - 1

// the first 16 bytes of every member this library writes (htslib's): FEXTRA, no time, XFL 0, OS unknown, XLEN 6, the
// subfield 'B' 'C' of 2 bytes; BSIZE follows
BGZF_HD uint8_t bgzf_header_byte(uint32_t i) {
  return i == 0 ? 0x1f : i == 1 ? 0x8b : i == 2 ? 8 : i == 3 ? 4 : i == 9 ? 0xff : i == 10 ? 6 : i == 12 ? 0x42 : i == 13 ? 0x43 : i == 14 ? 2 : 0;
}
// ... and the canonical 28-byte EOF marker: that header, BSIZE = 27, an empty fixed block, CRC-32 and ISIZE of nothing
BGZF_HD uint8_t bgzf_eof_byte(uint32_t i) { return i < 16 ? bgzf_header_byte(i) : i == 16 ? 0x1b : i == 18 ? 0x03 : 0; }

// The four bytes every member starts with: ID1 ID2, CM = 8, FLG with FEXTRA set and the reserved bits zero.  (What
// the discovery pass tests at every offset before it looks further.)
BGZF_HD bool bgzf_magic_ok(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t flg) {
  return b0 == 0x1f && b1 == 0x8b && b2 == 8 && (flg & 4u) != 0 && (flg & 0xe0u) == 0;
}

// THE MEMBER RULE.  m: the bytes at file offset p; avail = in_len - p, how many of them exist.  Returns the member's
// total size (BSIZE + 1), or 0: no member can be read at p.  A member has all of: the magic above; XLEN >= 6; inside
// the XLEN bytes a well-formed run of subfields (SI1 SI2 SLEN data, none running past XLEN), the first of which with
// SI = 'B' 'C' and SLEN = 2 gives BSIZE; total >= 12 + XLEN + 8; total <= avail.  FNAME, FCOMMENT and FHCRC are not
// examined: BSIZE alone moves the walk.  No byte at or behind m + avail is read; the loop makes at most XLEN / 4 steps.
BGZF_HD uint32_t bgzf_member_total(const uint8_t *m, uint64_t avail) {
  if (avail < 12u + 6u + kBgzfTrailerLen) return 0;
  if (!bgzf_magic_ok(m[0], m[1], m[2], m[3])) return 0;
  const uint32_t xlen = m[10] | ((uint32_t)m[11] << 8);
  if (xlen < 6u || avail < 12ull + xlen + kBgzfTrailerLen) return 0;
  const uint8_t *x = m + 12;
  uint32_t q = 0, total = 0;
  while (q < xlen) {
    if (q + 4u > xlen) return 0;  // a subfield header cut by XLEN
    const uint32_t slen = x[q + 2] | ((uint32_t)x[q + 3] << 8);
    if (q + 4u + slen > xlen) return 0;  // a subfield running past XLEN
    if (!total && x[q] == 0x42 && x[q + 1] == 0x43 && slen == 2u) total = (x[q + 4] | ((uint32_t)x[q + 5] << 8)) + 1u;
    q += 4u + slen;
  }
  if (!total || total < 12u + xlen + kBgzfTrailerLen || total > avail) return 0;
  return total;
}

// Is the member of `total` bytes at m the canonical EOF marker?
BGZF_HD bool bgzf_is_eof_marker(const uint8_t *m, uint32_t total) {
  if (total != kBgzfEofLen) return false;
  for (uint32_t i = 0; i < kBgzfEofLen; ++i)
    if (m[i] != bgzf_eof_byte(i)) return false;
  return true;
}

// The serial walk from offset 0: the specification of flate_hip_bgzf_index, and what the discovery kernels must equal
// on every input.  Returns 0 or FLATE_HIP_E_CORRUPT's value (-4); *n = the well-formed members in front of *err_off
// (-1 when the chain ends at in_len).  member_off (may be null): n + 1 entries when the walk succeeds.
inline int bgzf_serial_walk(const uint8_t *in, uint64_t in_len, uint64_t *n, int64_t *err_off, uint64_t *member_off) {
  uint64_t p = 0, k = 0;
  *err_off = -1;
  while (p < in_len) {
    const uint32_t t = bgzf_member_total(in + p, in_len - p);
    if (!t) {
      *n = k, *err_off = (int64_t)p;
      return -4;
    }
    if (member_off) member_off[k] = p;
    ++k, p += t;
  }
  if (member_off) member_off[k] = in_len;
  *n = k;
  return 0;
}

}  // namespace flate
