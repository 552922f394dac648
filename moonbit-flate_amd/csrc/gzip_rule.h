// gzip_rule.h -- where the members of a plain multi-member gzip file (RFC 1952: `cat a.gz b.gz`, rotated logs, WARC
// records) can start and how they chain, written ONCE: plain C++17 without HIP, compiled into the discovery kernels
// (gzip_kernels.hip), into the library's host code and into tests/host_model/gzip_rule_model.cpp, which compares it
// with the walk of tests/gzip_ref.py.
//
// Unlike a BGZF member, a gzip member does not say how long it is: its end is where its DEFLATE stream's final block
// ends, plus the 8-byte trailer.  So every offset that can start a member (gzip_header_len != 0) is a CANDIDATE, every
// candidate is decoded size-only over the range it is given, and the decode's verdict -- status s, output size z, and
// `used`, the bytes of the raw stream up to and including the byte that holds the last bit of the final block -- links
// it to the candidate at its end.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define GZIP_HD __host__ __device__ inline
#else
#define GZIP_HD inline
#endif

namespace flate {

constexpr uint32_t kGzipFixedLen = 10;    // ID1 ID2 CM FLG MTIME(4) XFL OS
constexpr uint32_t kGzipTrailerLen = 8;   // CRC-32, ISIZE
// the range a candidate is given, at most (option "gzip_member_max"): below 2^28 bytes, so that the 32-bit bit
// positions of the sub-block decoder hold
constexpr uint64_t kGzipMemberMax = (1ull << 28) - 1;
// the status words of the walk (FLATE_HIP_E_*; this header is compiled without flate_hip.h)
constexpr int kGzipOutTooSmall = -2, kGzipCorrupt = -4, kGzipTooLarge = -6, kGzipEof = -7;

// The three bytes every member starts with and the reserved FLG bits: what the discovery pass tests at every offset
// before it looks further.
GZIP_HD bool gzip_magic_ok(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t flg) {
  return b0 == 0x1f && b1 == 0x8b && b2 == 8 && (flg & 0xe0u) == 0;
}

// THE HEADER RULE (what frame_parse_kernel applies to a gzip member).  m: the bytes of the range, len of them.  Returns
// the header's length, or 0: no member can start here.  A member has: 1f 8b 08; FLG with the reserved bits zero; the
// ten fixed bytes; FEXTRA (XLEN, then that many bytes), FNAME and FCOMMENT (each up to and including a NUL, which must
// lie below len) and FHCRC (two bytes) skipped in that order; len >= header + 8.  No byte at or behind m + len is read.
GZIP_HD uint64_t gzip_header_len(const uint8_t *m, uint64_t len) {
  if (len < kGzipFixedLen || !gzip_magic_ok(m[0], m[1], m[2], m[3])) return 0;
  const uint32_t flg = m[3];
  uint64_t p = kGzipFixedLen;
  if (flg & 4u) {  // FEXTRA
    if (len < p + 2) return 0;
    p += 2u + (uint64_t)(m[p] | ((uint32_t)m[p + 1] << 8));
  }
  for (uint32_t bit = 8u; bit <= 16u; bit <<= 1) {  // FNAME, FCOMMENT: zero-terminated
    if (!(flg & bit)) continue;
    while (p < len && m[p]) ++p;
    if (p >= len) return 0;
    ++p;
  }
  if (flg & 2u) p += 2;  // FHCRC
  if (p > len || len < p + kGzipTrailerLen) return 0;
  return p;
}

// where candidate p's range ends: in[p, min(in_len, p + member_max))
GZIP_HD uint64_t gzip_range_end(uint64_t p, uint64_t in_len, uint64_t member_max) {
  return in_len - p > member_max ? p + member_max : in_len;
}

// What the walk makes of a candidate whose size-only decode ended with status s != 0: a stream that met the end of a
// range that member_max clipped is "too large" (such a member is read with flate_hip_inflate_stream_read), and so is
// one that inflates to 4 GiB or more (the decoders count output in 32 bits and report it as a slot that is too small).
GZIP_HD int gzip_dead_code(int s, uint64_t p, uint64_t in_len, uint64_t member_max) {
  if (s == kGzipOutTooSmall) return kGzipTooLarge;
  if (s == kGzipEof && in_len - p > member_max) return kGzipTooLarge;
  return s;
}

// One candidate of the table the walk reads: its offset and the verdict of its size-only decode over
// in[off + header, gzip_range_end(off) - 8).
struct GzipCand {
  uint64_t off;
  uint64_t used;  // bytes of the raw stream consumed (meaningful when s == 0)
  uint64_t z;     // bytes it inflates to (meaningful when s == 0)
  int32_t s;
};

// The serial walk from offset 0: the specification of flate_hip_gzip_index, and what the discovery kernels must equal
// on every input.  cand: the table, n_cand entries in rising order of off, one for every offset p with
// gzip_header_len(in + p, gzip_range_end(p) - p) != 0.  Returns 0 or the FLATE_HIP_E_* value that ended the walk; *n =
// the good members in front of *err_off (-1 when the chain ends at in_len).  member_off / out_off (may be null): *n + 1
// entries each, also when the walk fails -- the good prefix.
inline int gzip_serial_walk(const uint8_t *in, uint64_t in_len, uint64_t member_max, const GzipCand *cand, uint64_t n_cand,
                            uint64_t *n, int64_t *err_off, uint64_t *member_off, uint64_t *out_off) {
  uint64_t p = 0, k = 0, total = 0;
  int rc = 0;
  *err_off = -1;
  while (p < in_len) {
    const uint64_t hl = gzip_header_len(in + p, gzip_range_end(p, in_len, member_max) - p);
    uint64_t lo = 0, hi = n_cand;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (cand[mid].off < p) lo = mid + 1;
      else hi = mid;
    }
    if (!hl || lo == n_cand || cand[lo].off != p) {  // no member can start here
      rc = kGzipCorrupt;
      break;
    }
    if (cand[lo].s != 0) {
      rc = gzip_dead_code(cand[lo].s, p, in_len, member_max);
      break;
    }
    if (member_off) member_off[k] = p, out_off[k] = total;
    ++k, total += cand[lo].z, p += hl + cand[lo].used + kGzipTrailerLen;
  }
  if (rc) *err_off = (int64_t)p;
  if (member_off) member_off[k] = p, out_off[k] = total;
  *n = k;
  return rc;
}

}  // namespace flate
