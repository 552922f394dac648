// gzfile_seek_rule.h -- the seek index of a gzip FILE of any members (flate_hip_gzfile_seek_index / _ranges), written
// ONCE: plain C++17 without HIP, compiled into the kernels (gzfile_seek_kernels.hip), into the library's host code and
// into tests/host_model/gzfile_seek_rule_model.cpp, which compares it with tests/gzfile_seek_ref.py.
//
// n, unit_bit[0 .. n] (bits counted from the FILE's first byte), out_off[0 .. n], m, member_off[0 .. m] and
// member_unit[0 .. m] are flate_hip_gzfile_index's; T = out_off[n]; f(k) is the first unit of unit k's member.
//
// THE POINT RULE.  Unit k is a POINT iff k == 0, or k starts a member, or out_off[k] / span > out_off[k - 1] / span.
// pstart(k) and segments are seek_index_rule.h's, so a segment never crosses a member; with kSeekSpanNone the points
// are exactly the member starts.
//
// THE WINDOWS.  A point that starts a member has NO window: history never crosses a member.  Every other point p with
// unit u has one block of kSeekWindow bytes, block number p - j, j = upper_bound(member_unit[0 .. m), u) -- derived,
// never stored --, so there are n_points - m blocks.  A block holds the 32 KiB of ITS MEMBER's output in front of
// unit u in stream order; the bytes in front of the member's first byte are 0.
//
// THE INDEX, as 64-bit words: kGzSeekHeadWords of head (the kGzSeek* positions below), unit_bit[n + 1],
// out_off[n + 1], member_off[m + 1], member_unit[m + 1], point_unit[n_points].  An empty file: the head alone.
#pragma once

#include <stdint.h>

#include "seek_index_rule.h"

namespace flate {

constexpr uint64_t kGzSeekMagic = 0x58444953465a4746ull;  // "FGZFSIDX", little endian
constexpr uint64_t kGzSeekVersion = 1;
constexpr uint64_t kGzSeekHeaderMin = 10, kGzSeekTrailer = 8;  // a member's header is at least 10 bytes, its trailer 8
// the head's words
constexpr uint32_t kGzSeekMagicAt = 0, kGzSeekVersionAt = 1, kGzSeekInLenAt = 2, kGzSeekTotalAt = 3, kGzSeekSpanAt = 4,
                   kGzSeekUnitsAt = 5, kGzSeekMembersAt = 6, kGzSeekPointsAt = 7, kGzSeekRuleAt = 8,
                   kGzSeekHeadWords = 16;  // (9 .. 15: 0)
// word kGzSeekRuleAt: the unit rule the index was built with, kSeekRuleDynamic or kSeekRuleStored (seek_index_rule.h)

// the member of unit k: the last one whose first unit is at or in front of k (member_unit[0] == 0)
BGZF_HD uint32_t gzfile_seek_member_of(const uint64_t *member_unit, uint32_t m, uint32_t k) {
  return bgzf_upper_bound(member_unit, m, k) - 1u;
}
// THE POINT RULE for unit k (span >= 1: seek_span's result)
BGZF_HD bool gzfile_seek_is_point(const uint64_t *out_off, uint32_t k, uint64_t span, bool starts_member) {
  return starts_member || seek_is_point(out_off, k, span);
}
// the block of the window-bearing point p with unit u
BGZF_HD uint32_t gzfile_seek_block(const uint64_t *member_unit, uint32_t m, uint32_t p, uint32_t u) {
  return p - bgzf_upper_bound(member_unit, m, u);
}
// the window-bearing points in front of point p with unit u (a member start itself bears none)
BGZF_HD uint32_t gzfile_seek_blocks_before(const uint64_t *member_unit, uint32_t m, uint32_t p, uint32_t u) {
  const uint32_t j = bgzf_upper_bound(member_unit, m, u);  // (>= 1: member_unit[0] == 0)
  return p - j + (member_unit[j - 1u] == u ? 1u : 0u);
}
// what the decode of unit k needs
BGZF_HD uint64_t gzfile_seek_rel(const uint64_t *out_off, const uint64_t *member_unit, uint32_t m, uint32_t k) {
  return out_off[k] - out_off[member_unit[gzfile_seek_member_of(member_unit, m, k)]];
}
BGZF_HD uint32_t gzfile_seek_dict_len(uint64_t rel) { return rel < (uint64_t)kSeekWindow ? (uint32_t)rel : kSeekWindow; }
// unit k runs to BFINAL iff k + 1 starts a member or k + 1 == n (member_unit[m] == n)
BGZF_HD bool gzfile_seek_runs_to_final(const uint64_t *member_unit, uint32_t m, uint32_t k) {
  return member_unit[bgzf_upper_bound(member_unit, m, k)] == (uint64_t)k + 1u;
}

BGZF_HD uint64_t gzfile_seek_index_words(uint64_t n, uint64_t m, uint64_t n_points) {
  return n ? kGzSeekHeadWords + 2u * (n + 1u) + 2u * (m + 1u) + n_points : kGzSeekHeadWords;
}
BGZF_HD uint64_t gzfile_seek_windows_bytes(uint64_t n_points, uint64_t m) {
  return n_points > m ? (n_points - m) * kSeekWindow : 0ull;
}

// One range as the locate step leaves it: seek_locate over out_off and point_unit; ranges may cross members.
BGZF_HD SeekLoc gzfile_seek_locate(uint64_t begin, uint64_t end, const uint64_t *out_off, uint32_t n,
                                   const uint64_t *point_unit, uint32_t n_points) {
  return seek_locate(begin, end, out_off, n, point_unit, n_points);
}

// Verdict 1 of flate_hip_gzfile_ranges: the index describes SOME gzip file of in_len bytes, and the arrays are what
// the counts imply.  Host, O(n + m); nothing outside index[0, index_words) is read.
inline bool gzfile_seek_index_ok(const uint64_t *index, uint64_t index_words, uint64_t windows_bytes, uint64_t in_len) {
  if (!index || index_words < kGzSeekHeadWords) return false;
  if (index[kGzSeekMagicAt] != kGzSeekMagic || index[kGzSeekVersionAt] != kGzSeekVersion) return false;
  if (index[kGzSeekInLenAt] != in_len) return false;
  const uint64_t T = index[kGzSeekTotalAt], span = index[kGzSeekSpanAt], n = index[kGzSeekUnitsAt],
                 m = index[kGzSeekMembersAt], np = index[kGzSeekPointsAt];
  if (n == 0u)  // the empty file
    return m == 0u && np == 0u && in_len == 0u && T == 0u && index_words == kGzSeekHeadWords && windows_bytes == 0u;
  if (n >= 0xffffffffull || m < 1u || m > n || np < m || np > n || span < 1u) return false;
  if (index_words != gzfile_seek_index_words(n, m, np) || windows_bytes != gzfile_seek_windows_bytes(np, m)) return false;
  if (in_len > (~0ull >> 3)) return false;
  const uint64_t *unit_bit = index + kGzSeekHeadWords, *out_off = unit_bit + (n + 1u), *member_off = out_off + (n + 1u),
                 *member_unit = member_off + (m + 1u), *point_unit = member_unit + (m + 1u);
  if (out_off[0] != 0u || out_off[n] != T) return false;
  if (member_off[0] != 0u || member_off[m] != in_len || member_unit[0] != 0u || member_unit[m] != n) return false;
  for (uint64_t k = 0; k < n; ++k)
    if (unit_bit[k + 1u] <= unit_bit[k] || out_off[k + 1u] < out_off[k]) return false;
  for (uint64_t j = 0; j < m; ++j) {
    if (member_off[j + 1u] <= member_off[j] || member_off[j + 1u] - member_off[j] < kGzSeekHeaderMin + kGzSeekTrailer)
      return false;
    if (member_unit[j + 1u] <= member_unit[j] || member_unit[j + 1u] > n) return false;
  }
  // every member's units lie inside it, and no unit is longer than kSeekUnitBitsMax
  for (uint64_t j = 0; j < m; ++j) {
    const uint64_t lo = member_unit[j], hi = member_unit[j + 1u], end_bit = 8u * (member_off[j + 1u] - kGzSeekTrailer);
    if (unit_bit[lo] < 8u * (member_off[j] + kGzSeekHeaderMin) || unit_bit[hi - 1u] >= end_bit) return false;
    for (uint64_t k = lo; k < hi; ++k) {
      const uint64_t stop = k + 1u < hi ? unit_bit[k + 1u] : end_bit;
      if (stop - unit_bit[k] > kSeekUnitBitsMax) return false;
    }
  }
  uint64_t p = 0, j = 0;
  for (uint64_t k = 0; k < n; ++k) {
    const bool starts = j < m && member_unit[j] == k;
    if (starts) ++j;
    if (gzfile_seek_is_point(out_off, (uint32_t)k, span, starts)) {
      if (p >= np || point_unit[p] != k) return false;
      ++p;
    }
  }
  return p == np;
}

// ... and, for an index that passed gzfile_seek_index_ok: its unit rule is one this library walks by
inline bool gzfile_seek_index_rule_ok(const uint64_t *index) {
  return index[kGzSeekRuleAt] == kSeekRuleDynamic || index[kGzSeekRuleAt] == kSeekRuleStored;
}

}  // namespace flate
