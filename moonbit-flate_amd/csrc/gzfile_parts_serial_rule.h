// gzfile_parts_serial_rule.h -- a gzip FILE read in PARTS with short members decoded WHOLE inside a part
// (flate_hip_gzfile_reader_set_serial_max: S >= 1), written ONCE: plain C++17 without HIP, compiled into the kernels
// (gzfile_parts_serial_kernels.hip, gzfile_kernels.hip), into the library's host code and into
// tests/host_model/gzfile_parts_serial_rule_model.cpp, which compares it with tests/gzfile_parts_serial_ref.py.
//
// The same kernels run the whole file ("gzfile_serial_max"), which is the part that is final and starts at a BOUNDARY,
// with out_cap = ~0.  Three equalities carry that, and the model sweeps them: gzfile_parts_hop(.., true) is gzfile_hop;
// gzfile_parts_serial_verdict(in_len, true, S, ~0, ..) is WHOLE exactly where gzfile_serial_whole holds, LONG elsewhere
// and never OPEN; gzfile_parts_serial_from(in_len, false, none, off, v != OPEN, ..) is in_len if none, else off, with
// no OPEN stop -- gzfile_serial_walk's find_from.
//
// It joins gzfile_serial_rule.h (the serial range, the whole test, the record of a whole member) and
// gzfile_parts_rule.h (THE PARTS HOP, the call) over one part in[0, in_len): every offset p that passes the header rule
// over in[p, in_len) gets the serial range of the PART -- E = min(in_len - 8, p + S), the probes of every part read
// in[.., in_len - 8) -- and ONE size-only launch of the batch decoders runs over all of them.  A candidate then has one
// of THREE VERDICTS:
//   WHOLE  gzfile_serial_whole holds and the member inflates to at most the call's out_cap bytes: one unit, decoded by
//          the batch decoders.  (A larger member is cut into units, so that a bounded output buffer makes the progress
//          it makes with S = 0.)
//   OPEN   the part is not final, the range was clipped by the part and not by S (in_len - 8 < p + S) and the decode ran
//          out of input there (FLATE_HIP_E_UNEXPECTED_EOF, or the header alone did not fit in front of E): more bytes
//          could still make the member whole.
//   LONG   everything else: cut into units exactly as with S = 0.
// THE WALK at a BOUNDARY goes from the member at byte 0 along THE PARTS HOP for as long as members are WHOLE; where it
// rests says where FIND starts (find_from).  A hop that lands on the header of an OPEN member at p > 0 is a BOUNDARY
// stop at p (the next part judges that member as its root); an OPEN member at the root is LONG, so that the reader
// never needs a part of a minimum size.  INSIDE a member find_from is 0: the continued member is units.
#pragma once

#include <stdint.h>

#include "gzfile_parts_rule.h"
#include "gzfile_serial_rule.h"

namespace flate {

constexpr uint32_t kGzPartLong = 0, kGzPartWhole = 1, kGzPartOpen = 2;

// THE THREE VERDICTS of the candidate at p (header length hl, or 0) whose size-only decode over
// [gzfile_serial_begin, E) left status / used / out.
GZIP_HD uint32_t gzfile_parts_serial_verdict(uint64_t in_len, bool final_in, uint64_t S, uint64_t out_cap, uint64_t p,
                                             uint64_t hl, int32_t status, uint64_t used, uint64_t out) {
  const uint64_t E = gzfile_serial_end(in_len, p, S);
  if (gzfile_serial_whole(status, p, hl, used, E)) return out <= out_cap ? kGzPartWhole : kGzPartLong;
  if (final_in) return kGzPartLong;
  const uint64_t raw_end = in_len >= kGzipTrailerLen ? in_len - kGzipTrailerLen : 0ull;
  const bool by_part = raw_end < p + S;  // (p + S < 2^63: p is a part offset, S < 2^28)
  const bool ran_out = hl == 0 || p + hl > E || status == kPartsEof;
  return by_part && ran_out ? kGzPartOpen : kGzPartLong;
}

// THE LINK behind a final block that ends at bit b: THE PARTS HOP, except that a hop onto the header of an OPEN member
// is a BOUNDARY stop there.  verdict_at(e): the verdict of the candidate whose header starts at e (a hop's target has
// passed the header rule, so it is one; e > 0).
template <class VerdictAt>
GZIP_HD GzHop gzfile_parts_serial_hop(const uint8_t *in, uint64_t in_len, uint64_t b, bool final_in, VerdictAt verdict_at) {
  GzHop h = gzfile_parts_hop(in, in_len, b, final_in);
  if (h.kind == kGzHopNext && verdict_at(h.e) == kGzPartOpen) h.kind = kGzHopStop;
  return h;
}

// Where FIND starts, from where the walk over the WHOLE members came to rest: rest_off / rest_verdict are the offset
// and the verdict of the first member on the walk that is not whole; none = the walk reached the file's end, a dead hop
// or a stop, or the part starts with no member.  *open_stop: the walk ended in front of an OPEN member.
GZIP_HD uint64_t gzfile_parts_serial_from(uint64_t in_len, bool inside, bool none, uint64_t rest_off, uint32_t rest_verdict,
                                          uint32_t *open_stop) {
  *open_stop = 0u;
  if (inside) return 0ull;
  if (none) return in_len;
  if (rest_verdict == kGzPartOpen && rest_off > 0ull) {
    *open_stop = 1u;
    return in_len;
  }
  return rest_off;  // LONG, or OPEN at the root
}

// THE WALK on the host (the model's; the kernels double pointers over the same links).  cand: n_cand entries in rising
// order of off, one for every offset that passes the header rule over in[off, in_len), with what the size-only decode
// over its serial range left.  -> find_from; *n_whole = the whole members passed, *open_stop as above.
inline uint64_t gzfile_parts_serial_walk(const uint8_t *in, uint64_t in_len, bool final_in, bool inside, uint64_t S,
                                         uint64_t out_cap, const GzSerialCand *cand, uint64_t n_cand, uint64_t *n_whole,
                                         uint32_t *open_stop) {
  *n_whole = 0;
  auto at = [&](uint64_t p) -> uint64_t {
    uint64_t lo = 0, hi = n_cand;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (cand[mid].off < p) lo = mid + 1;
      else hi = mid;
    }
    return lo < n_cand && cand[lo].off == p ? lo : n_cand;
  };
  auto verdict = [&](uint64_t j) {
    const uint64_t p = cand[j].off;
    return gzfile_parts_serial_verdict(in_len, final_in, S, out_cap, p, gzip_header_len(in + p, in_len - p), cand[j].s,
                                       cand[j].used, cand[j].z);
  };
  if (inside) return gzfile_parts_serial_from(in_len, true, true, 0, 0, open_stop);
  uint64_t p = 0;
  for (uint64_t step = 0; step <= n_cand; ++step) {
    const uint64_t j = p < in_len ? at(p) : n_cand;
    if (j == n_cand) break;  // (only at p == 0: a hop's target passed the rule)
    const uint32_t v = verdict(j);
    if (v != kGzPartWhole) return gzfile_parts_serial_from(in_len, false, false, p, v, open_stop);
    ++*n_whole;
    const uint64_t hl = gzip_header_len(in + p, in_len - p);
    const GzHop h = gzfile_parts_hop(in, in_len, gzfile_serial_record(p, hl, cand[j].used, cand[j].z).end_bit, final_in);
    if (h.kind != kGzHopNext) break;
    p = h.e;  // (an OPEN member there ends the walk in the next step)
  }
  return gzfile_parts_serial_from(in_len, false, true, 0, 0, open_stop);
}

// THE CALL with S >= 1: gzfile_parts_call, except that a call whose first undelivered unit is a member's first unit
// stops at the BOUNDARY in front of that member's HEADER (*in_used = the header's offset), not INSIDE behind it -- the
// next part then judges that member as a root.  S == 0: gzfile_parts_call.
inline GzPartsCall gzfile_parts_serial_call(const GzPartsState &s, const GzPartsIndex &X, uint64_t in_len, bool final_in,
                                            uint64_t out_cap, uint64_t unit_max, uint64_t S) {
  GzPartsCall c = gzfile_parts_call(s, X, in_len, final_in, out_cap, unit_max);
  if (!S || c.plan.action != kPartsDecode || c.plan.terminal || !X.u_start[c.plan.n_del]) return c;
  c.in_used = X.u_start[c.plan.n_del] - 1u;
  GzPartsState &t = c.next;
  t.inside = 0, t.b0 = 0, t.produced = 0;
  t.consumed = s.consumed + c.in_used;
  return c;
}

// the whole members among the first n units (u_whole: the discovery's per-unit marks)
inline uint32_t gzfile_parts_serial_count(const uint32_t *u_whole, uint32_t n) {
  uint32_t k = 0;
  for (uint32_t u = 0; u < n; ++u) k += u_whole[u] ? 1u : 0u;
  return k;
}

// a handle is FRESH after open or reset, until a call has consumed a byte or ended the file
inline bool gzfile_parts_is_fresh(const GzPartsState &s) { return s.consumed == 0 && s.status == 0 && !s.inside; }

// ---- the arguments (api_checks.h hands them on) ----
ONE_PARTS_HD int gzfile_parts_serial_set_args(const void *r, uint64_t S, bool fresh) {
  if (!r || S > kGzSerialMax || !fresh) return kPartsInvalid;
  return kPartsOk;
}
ONE_PARTS_HD int gzfile_parts_route_args(const void *r, const void *serial_members, const void *open_stop,
                                         const void *find_from) {
  if (!r || !serial_members || !open_stop || !find_from) return kPartsInvalid;
  return kPartsOk;
}

}  // namespace flate
