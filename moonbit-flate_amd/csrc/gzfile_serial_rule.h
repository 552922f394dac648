// gzfile_serial_rule.h -- which members of a gzip FILE are decoded WHOLE (flate_hip_gzfile_index / _read with the
// option "gzfile_serial_max" = S >= 1), written ONCE: plain C++17 without HIP, compiled into the kernels
// (gzfile_serial_kernels.hip; the walk's, through gzfile_parts_serial_rule.h), into the library's host code and into
// tests/host_model/gzfile_serial_rule_model.cpp, which compares it with the model of tests/gzfile_serial_ref.py.
//
// A member whose header starts at byte p and is hl bytes long is given the SERIAL RANGE in[p + hl, E) with
// E = min(in_len - 8, p + S): the file's last 8 bytes can only be a trailer, and header and raw stream together get
// at most S bytes.  The member is WHOLE iff a size-only serial decode over that range reaches the end of its final
// block with status 0 (so not FLATE_HIP_E_UNEXPECTED_EOF at the clip, not a bad distance, not 4 GiB of output or
// more) and p + hl + used <= E, `used` being the bytes consumed up to and including the byte that holds the last bit of
// the final block (InfParams::used).  A whole member is ONE node of the file's chain: it is never searched for block
// headers and never walked symbolically.  Its record is a good probe's that ended with BFINAL at the byte-rounded bit
// 8 * (p + hl + used); its link is THE HOP of gzfile_rule.h from there, unchanged -- the hop rounds up to the byte, so
// the rounded bit gives the same `e` as the true one.
#pragma once

#include <stdint.h>

#include "gzfile_rule.h"

namespace flate {

// the option's largest value: the range of the sub-block decoder's 32-bit bit positions, as for "gzip_member_max"
constexpr uint64_t kGzSerialMax = (1ull << 28) - 1;

// E: where the serial range of the member at p ends (S >= 1).  A p at or behind in_len - 8 has no range: E <= p.
GZIP_HD uint64_t gzfile_serial_end(uint64_t in_len, uint64_t p, uint64_t S) {
  const uint64_t raw_end = in_len >= kGzipTrailerLen ? in_len - kGzipTrailerLen : 0ull;
  if (p >= raw_end) return raw_end;
  return raw_end - p > S ? p + S : raw_end;
}

// the range the size-only decode of the member at p is given: [lo, E), empty (lo == E) when the header alone does not
// fit -- the decoders then meet the end of the stream at once and the member is not whole.  hl: gzip_header_len, or 0.
GZIP_HD uint64_t gzfile_serial_begin(uint64_t p, uint64_t hl, uint64_t E) {
  return (hl != 0 && p + hl <= E) ? p + hl : E;
}

// THE WHOLE TEST.  status / used: what the size-only decode over [gzfile_serial_begin, E) left.
GZIP_HD bool gzfile_serial_whole(int32_t status, uint64_t p, uint64_t hl, uint64_t used, uint64_t E) {
  return status == 0 && hl != 0 && p + hl <= E && used <= E - (p + hl);
}

// The node record of a whole member, field for field an OneProbe (flate_kernels.h).
struct GzSerialRecord {
  uint64_t end_bit;      // 8 * (p + hl + used): the byte behind the final block
  uint64_t out;          // what the member inflates to
  int64_t err_off;       // -1
  int32_t status;        // 0
  uint32_t final_block;  // 1
};
GZIP_HD GzSerialRecord gzfile_serial_record(uint64_t p, uint64_t hl, uint64_t used, uint64_t out) {
  GzSerialRecord r;
  r.end_bit = 8u * (p + hl + used);
  r.out = out;
  r.err_off = -1;
  r.status = 0;
  r.final_block = 1u;
  return r;
}

// One candidate of List B as the walk reads it: its header's offset and the verdict of its size-only decode over its
// serial range.
struct GzSerialCand {
  uint64_t off;
  uint64_t used;  // (meaningful when s == 0)
  uint64_t z;     // bytes it inflates to (meaningful when s == 0)
  int32_t s;
};

// THE SERIAL WALK: from the member at offset 0 along the hops for as long as the members it reaches are whole.
// cand: n_cand entries in rising order of off, one for every offset that passes the header rule over in[off, in_len).
// Returns find_from: the offset of the first member on the walk that is not whole, or in_len when the walk reaches the
// file's end, a dead hop or a file that starts with no member -- no bit-offset search is needed then.  *n_whole = the
// whole members it passed.  Every step lands above the trailer it skips: at most n_cand steps.
inline uint64_t gzfile_serial_walk(const uint8_t *in, uint64_t in_len, uint64_t S, const GzSerialCand *cand,
                                   uint64_t n_cand, uint64_t *n_whole) {
  uint64_t p = 0;
  *n_whole = 0;
  for (uint64_t step = 0; step <= n_cand; ++step) {
    if (p >= in_len) return in_len;
    uint64_t lo = 0, hi = n_cand;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (cand[mid].off < p) lo = mid + 1;
      else hi = mid;
    }
    if (lo == n_cand || cand[lo].off != p) return in_len;  // (only at p == 0: a hop's target passed the rule)
    const uint64_t hl = gzip_header_len(in + p, in_len - p);
    const uint64_t E = gzfile_serial_end(in_len, p, S);
    if (!gzfile_serial_whole(cand[lo].s, p, hl, cand[lo].used, E)) return p;
    ++*n_whole;
    const GzHop h = gzfile_hop(in, in_len, gzfile_serial_record(p, hl, cand[lo].used, cand[lo].z).end_bit);
    if (h.kind != kGzHopNext) return in_len;
    p = h.e;
  }
  return in_len;
}

}  // namespace flate
