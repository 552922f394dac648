// bgzf_range_rule.h -- where a range of flate_hip_bgzf_read_ranges lies in a BGZF file's uncompressed bytes, written
// ONCE: plain C++17 without HIP, compiled into the locate kernel (bgzf_range_kernels.hip), into the library's host code
// (the empty file, which has no index on the device) and into tests/host_model/bgzf_range_model.cpp, which compares it
// with tests/bgzf_range_ref.py.
//
// The index is flate_hip_bgzf_index's: member_off[0 .. n] (strictly increasing, member_off[n] = in_len) and
// out_off[0 .. n] (the exclusive prefix sum of the members' ISIZE, out_off[n] = T).
#pragma once

#include <stdint.h>

#include <vector>

#include "bgzf_rule.h"

namespace flate {

constexpr uint32_t kBgzfPosBytes = 0;    // FLATE_HIP_BGZF_POS_BYTES
constexpr uint32_t kBgzfPosVirtual = 1;  // FLATE_HIP_BGZF_POS_VIRTUAL
constexpr uint32_t kBgzfNoMember = 0xffffffffu;

// The first index i in [0, cnt] with a[i] > x (cnt: nothing is).  At most 33 steps.
BGZF_HD uint32_t bgzf_upper_bound(const uint64_t *a, uint32_t cnt, uint64_t x) {
  uint32_t lo = 0, hi = cnt;
  for (int it = 0; it < 33 && lo < hi; ++it) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (a[mid] <= x) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}
// The first index i in [0, cnt] with a[i] >= x.
BGZF_HD uint32_t bgzf_lower_bound(const uint64_t *a, uint32_t cnt, uint64_t x) {
  uint32_t lo = 0, hi = cnt;
  for (int it = 0; it < 33 && lo < hi; ++it) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (a[mid] < x) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}

// THE VALIDITY RULE of a virtual offset v = c << 16 | u: c is the start of member k (k == n: the end of the file) and
// u <= ISIZE[k] (k == n: u == 0).  A c that merely passes the member rule -- a decoy -- is not in member_off.
// Returns true and *pos = out_off[k] + u, or false.
BGZF_HD bool bgzf_virtual_pos(uint64_t v, const uint64_t *member_off, const uint64_t *out_off, uint32_t n, uint64_t *pos) {
  const uint64_t c = v >> 16, u = v & 0xffffu;
  const uint32_t k = bgzf_lower_bound(member_off, n + 1u, c);
  if (k > n || member_off[k] != c) return false;
  const uint64_t isize = k < n ? out_off[k + 1u] - out_off[k] : 0ull;
  if (u > isize) return false;
  *pos = out_off[k] + u;
  return true;
}

// One range as the locate step leaves it.
struct BgzfRangeLoc {
  uint64_t b, e;       // U[b, e): what the range delivers (b == e == 0 for an invalid range)
  int32_t status;      // 0, or FLATE_HIP_E_INVALID's value (-1): an invalid virtual offset
  uint32_t first, last;  // the first and the last member with bytes inside [b, e); kBgzfNoMember: there is none
};

// THE RANGE RULE.  kind: kBgzfPosBytes (clamped to T, as pread reads short) or kBgzfPosVirtual (the rule above).
// begin <= end numerically: the entry point has refused everything else.
BGZF_HD BgzfRangeLoc bgzf_range_locate(uint32_t kind, uint64_t begin, uint64_t end, const uint64_t *member_off,
                                       const uint64_t *out_off, uint32_t n) {
  BgzfRangeLoc r;
  r.b = r.e = 0;
  r.status = 0;
  r.first = r.last = kBgzfNoMember;
  const uint64_t T = out_off[n];
  if (kind == kBgzfPosVirtual) {
    uint64_t b = 0, e = 0;
    if (!bgzf_virtual_pos(begin, member_off, out_off, n, &b) || !bgzf_virtual_pos(end, member_off, out_off, n, &e) || b > e) {
      r.status = -1;
      return r;
    }
    r.b = b, r.e = e;
  } else {
    r.b = begin < T ? begin : T;
    r.e = end < T ? end : T;
  }
  if (r.b >= r.e) return r;
  // out_off repeats where members are empty: the member that HOLDS byte b is the last one that starts at or below it,
  // the member that holds byte e - 1 the last one that starts below e -- both have ISIZE > 0
  r.first = bgzf_upper_bound(out_off, n + 1u, r.b) - 1u;
  r.last = bgzf_lower_bound(out_off, n + 1u, r.e) - 1u;
  return r;
}

// THE STATUS RULE of a ranges call, behind the decode (host only).  st[0 .. ns): the statuses of the decoded members or
// units in file order; range r touches the decoded [r_lo[r], r_hi[r]).  A range takes the status of the first one it
// touches that has one; a range that touches none (r_lo[r] == r_hi[r]), that lies outside the decoded ones, or that was
// settled before the decode (skip != null and skip[r] != 0) keeps what it has.  range_status may be null.  Returns the
// first decoded one with a status -- the call's verdict is its status -- or ns: there is none.
inline uint32_t range_statuses(const int32_t *st, uint32_t ns, const uint32_t *r_lo, const uint32_t *r_hi, uint32_t nr,
                               int32_t *range_status, const int32_t *skip) {
  std::vector<uint32_t> nxt((size_t)ns + 1);  // nxt[i] = the first decoded one at or behind i with a status
  nxt[ns] = ns;
  for (uint32_t i = ns; i-- > 0;) nxt[i] = st[i] ? i : nxt[i + 1];
  if (range_status)
    for (uint32_t r = 0; r < nr; ++r)
      if (!(skip && skip[r]) && r_lo[r] < r_hi[r] && r_hi[r] <= ns && nxt[r_lo[r]] < r_hi[r]) range_status[r] = st[nxt[r_lo[r]]];
  return nxt[0];
}

}  // namespace flate
