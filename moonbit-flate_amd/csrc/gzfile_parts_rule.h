// gzfile_parts_rule.h -- a gzip FILE of any members read in PARTS (flate_hip_gzfile_reader_*), what a call decides,
// written ONCE: plain C++17 without HIP, compiled into the kernels (gzfile_kernels.hip, which run the whole file as the
// part that is final and starts at a BOUNDARY, and gzfile_parts_kernels.hip), into the library's host code and into
// tests/host_model/gzfile_parts_rule_model.cpp, which compares it with tests/gzfile_parts_ref.py.
//
// A call is flate_hip_gzfile_read's discovery and rounds over the part in[0, in_len) of the file.  Between two calls
// the reader stands at a BOUNDARY (the next part's first byte is where a header must stand, or the file's end) or
// INSIDE a member (the next unit starts at bit b0 of the next part's first byte).  There is no "trailer pending"
// state: the probes of every part read in[.., in_len - 8), so a final block that is complete has its trailer inside
// the part, and THE PARTS HOP says what stands behind it.  This file holds the hop, the root of a part's chain, which
// units a call delivers (one_parts_plan's policy), the members that end among them, what the handle remembers, and the
// result words of a failure, counted over the FILE.
#pragma once

#include <stdint.h>

#include <vector>

#include "gzfile_rule.h"
#include "one_parts_rule.h"

namespace flate {

constexpr uint32_t kGzHopStop = 3;  // (beside gzfile_rule.h's three) a BOUNDARY stop at byte e: the next part starts there

// THE PARTS HOP behind a final block that ends at bit b of the part (b <= 8 * (in_len - 8)).  On a final part it is
// gzfile_hop.  On any other part the bytes behind the trailer may be a header that the part cuts: the chain is dead
// only where a byte that is there already fails (later bytes cannot mend it), else the reader stops at e.
GZIP_HD GzHop gzfile_parts_hop(const uint8_t *in, uint64_t in_len, uint64_t b, bool final_in) {
  GzHop h;
  h.e = (b + 7u) / 8u + kGzipTrailerLen;
  h.bit = 0;
  if (h.e >= in_len) {
    h.kind = h.e > in_len ? kGzHopDead : final_in ? kGzHopEnd : kGzHopStop;
    return h;
  }
  h.bit = gzfile_first_bit(in, in_len, h.e);
  if (h.bit) {
    h.kind = kGzHopNext;
  } else if (final_in) {
    h.kind = kGzHopDead;
  } else {
    uint64_t hl = 0;
    h.kind = one_parts_header(kPartsGzip, in + h.e, in_len - h.e, &hl) == kPartsHdrBad ? kGzHopDead : kGzHopStop;
  }
  return h;
}

// THE ROOT of a part that starts at a BOUNDARY: the header at byte 0.  Good: a member starts here and its first unit at
// byte *hl (then gzip_header_len(in, in_len) == *hl: the List-B node at offset 0 exists).  More: refused only because
// the part ends here -- the header is cut, or fewer than 8 bytes stand behind it.  Bad: some byte fails.
ONE_PARTS_HD uint32_t gzfile_parts_root(const uint8_t *in, uint64_t in_len, uint64_t *hl) {
  uint32_t v = one_parts_header(kPartsGzip, in, in_len, hl);
  if (v == kPartsHdrGood && in_len < *hl + kGzipTrailerLen) v = kPartsHdrMore;
  return v;
}

// ---- what the handle remembers (host words; the device holds the window and the member's running CRC-32) ----
struct GzPartsState {
  uint64_t consumed;      // file bytes used so far: the sum of *in_used
  uint64_t member_off;    // INSIDE: the member's file offset ...
  uint64_t raw_off;       // ... its raw stream's file offset ...
  uint64_t produced;      // ... and the bytes it has produced
  uint32_t members_done;  // members whose trailers were judged good
  uint32_t inside;        // 0: BOUNDARY
  uint32_t b0;            // INSIDE: the next unit starts at this bit of the next part's first byte
  int32_t status;         // sticky: 0, FLATE_HIP_STREAM_END or the file's error, with the three words below
  uint32_t bad_member;
  int64_t err_off, stream_err_off;
};
inline GzPartsState gzfile_parts_fresh() { return GzPartsState{0, 0, 0, 0, 0, 0, 0, 0, 0xffffffffu, -1, -1}; }

// ---- the discovery over a part, as the host has read it back ----
struct GzPartsIndex {
  uint32_t n;               // good units
  const uint64_t *unit_bit; // n + 1: entry n = where the failing unit starts, or where the last good one ends
  const uint64_t *out_off;  // n + 1
  const uint64_t *u_start;  // n + 1: header offset + 1 of a unit that starts a member, else 0
  const uint32_t *u_final;  // n: the unit ends with BFINAL
  int rc;                   // the chain's verdict: 0 = it reached the file's end or a BOUNDARY stop
  int64_t err_off;          // part-relative
  uint32_t fail_unit;       // unit n fails behind its header after fail_out bytes
  uint64_t fail_out;
  uint32_t no_header;       // rc is "no member can start at err_off"
};

// a member (or the rest of the continued one) among the units a call decodes
struct GzPartSeg {
  uint64_t trailer_at;  // where its trailer stands in the part; ~0: it does not end among the delivered units
  uint64_t size;        // what the member inflates to, the bytes of earlier calls included (when it ends)
  uint64_t out_begin, out_end;  // its bytes of this call: out[out_begin, out_end)
  uint32_t first_unit, last_unit;
};

struct GzPartsCall {
  OnePartsPlan plan;            // kPartsDecode: the rest below is set
  std::vector<GzPartSeg> segs;  // in file order; all but the last end
  std::vector<uint64_t> bounds; // segs.size() + 1: the checksum launch's ranges
  uint32_t continued = 0;       // seg 0 is the member in progress
  uint32_t n_end = 0;           // members that end among the delivered units
  uint64_t in_used = 0;         // if nothing fails
  bool at_end = false;          // ... and the call is FLATE_HIP_STREAM_END
  GzPartsState next{};          // ... and this is the state behind it
};

// which member unit u of the part belongs to: its number over the file, its file offset and its raw stream's
struct GzPartsMember {
  uint32_t number;
  uint64_t off, raw_off;
};
inline GzPartsMember gzfile_parts_member(const GzPartsState &s, const GzPartsIndex &X, uint32_t u) {
  uint32_t c = 0, at = 0;
  for (uint32_t k = 0; k <= u && k <= X.n; ++k)
    if (X.u_start[k]) ++c, at = k;
  if (c == 0) return GzPartsMember{s.members_done, s.member_off, s.raw_off};
  return GzPartsMember{s.members_done + (s.inside ? c : c - 1u), s.consumed + X.u_start[at] - 1u,
                       s.consumed + X.unit_bit[at] / 8u};
}

// THE CALL: one_parts_plan over the chain's units, then the members among the delivered units, *in_used and the state.
inline GzPartsCall gzfile_parts_call(const GzPartsState &s, const GzPartsIndex &X, uint64_t in_len, bool final_in,
                                     uint64_t out_cap, uint64_t unit_max) {
  GzPartsCall c;
  c.plan = one_parts_plan(X.n, X.out_off, X.rc, X.fail_unit, X.fail_out, final_in, out_cap, in_len, unit_max);
  c.next = s;
  if (c.plan.action != kPartsDecode) return c;
  const OnePartsPlan &p = c.plan;
  const uint32_t n_dec = p.n_del + p.with_fail;
  std::vector<uint32_t> first;
  if (s.inside && n_dec) first.push_back(0u), c.continued = 1u;
  for (uint32_t k = 0; k < n_dec; ++k)
    if (X.u_start[k] && !(k == 0 && c.continued)) first.push_back(k);
  const size_t ns = first.size();
  for (size_t i = 0; i < ns; ++i) {
    GzPartSeg g{};
    g.first_unit = first[i];
    g.last_unit = (i + 1 < ns ? first[i + 1] : n_dec) - 1u;
    g.out_begin = X.out_off[g.first_unit];
    g.out_end = i + 1 < ns ? X.out_off[first[i + 1]] : p.total;
    g.trailer_at = ~0ull;
    if (g.last_unit < p.n_del && X.u_final[g.last_unit]) {  // the member ends here: its trailer lies in the part
      const uint32_t nx = g.last_unit + 1u;
      const uint64_t end = X.u_start[nx] ? X.u_start[nx] - 1u : (X.unit_bit[nx] + 7u) / 8u + kGzipTrailerLen;
      g.trailer_at = end - kGzipTrailerLen;
      g.size = g.out_end - g.out_begin + (i == 0 && c.continued ? s.produced : 0ull);
      ++c.n_end;
    }
    c.bounds.push_back(g.out_begin);
    c.segs.push_back(g);
  }
  c.bounds.push_back(p.total);
  if (ns) c.bounds[0] = 0;
  GzPartsState &t = c.next;
  if (p.terminal && X.rc != 0) return c;  // the file's failure: sticky, nothing used
  t.members_done += c.n_end;
  if (p.terminal) {  // the chain reached the file's end or a BOUNDARY stop
    c.in_used = (X.unit_bit[X.n] + 7u) / 8u + kGzipTrailerLen;
    c.at_end = final_in;
    t.inside = 0, t.b0 = 0, t.produced = 0;
  } else {
    const uint64_t bit = X.unit_bit[p.n_del];
    c.in_used = bit / 8u;
    t.inside = 1u;
    t.b0 = (uint32_t)(bit & 7u);
    if (X.u_start[p.n_del]) {  // a member's first unit: the trailer and the header in front are used
      t.member_off = s.consumed + X.u_start[p.n_del] - 1u;
      t.raw_off = s.consumed + bit / 8u;
      t.produced = 0;
    } else {
      const GzPartSeg &g = c.segs.back();
      if (ns == 1 && c.continued) {
        t.produced = s.produced + (g.out_end - g.out_begin);
      } else {
        t.member_off = s.consumed + X.u_start[g.first_unit] - 1u;
        t.raw_off = s.consumed + X.unit_bit[g.first_unit] / 8u;
        t.produced = g.out_end - g.out_begin;
      }
    }
  }
  t.consumed += c.in_used;
  return c;
}

// ---- the file's failure: the sticky words, counted over the FILE ----
// what the device reports behind the rounds: the status, and which of the three it is
struct GzPartsFail {
  int32_t status;
  uint32_t bad_trailer;  // a segment's number, or 0xffffffff
  uint32_t bad_unit;     // the unit TAIL failed in, or 0xffffffff: the chain's verdict (X.rc at X.err_off)
  int64_t err_off;       // part-relative (a unit's failure)
};
inline void gzfile_parts_fail(GzPartsState &s, const GzPartsIndex &X, const GzPartsCall &c, const GzPartsFail &f) {
  s.status = f.status;
  s.stream_err_off = -1;
  if (f.bad_trailer != 0xffffffffu) {
    const GzPartSeg &g = c.segs[f.bad_trailer];
    const GzPartsMember m = gzfile_parts_member(s, X, g.first_unit);
    s.bad_member = m.number;
    s.err_off = (int64_t)m.off;
    s.stream_err_off = (int64_t)(s.consumed + g.trailer_at + kGzipTrailerLen - m.off);
    return;
  }
  if (f.bad_unit == 0xffffffffu && X.no_header) {  // no member can start behind the last one's trailer
    s.bad_member = s.members_done + c.n_end;
    s.err_off = (int64_t)s.consumed + X.err_off;
    return;
  }
  const uint32_t u = f.bad_unit != 0xffffffffu ? f.bad_unit : X.n;
  const int64_t eo = f.bad_unit != 0xffffffffu ? f.err_off : X.err_off;
  const GzPartsMember m = gzfile_parts_member(s, X, u);
  s.bad_member = m.number;
  s.err_off = (int64_t)m.off;
  if (f.status == kPartsCorrupt && eo >= 0) s.stream_err_off = (int64_t)s.consumed + eo - (int64_t)m.raw_off;
}

// ---- the arguments (api_checks.h hands them on) ----
ONE_PARTS_HD int gzfile_parts_open_args(const void *ctx, uint32_t flags, uint32_t device_ptrs, const void *r) {
  if (!ctx || !r || (flags & ~device_ptrs)) return kPartsInvalid;
  return kPartsOk;
}

}  // namespace flate
