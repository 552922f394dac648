// seek_index_rule.h -- the seek index of ONE long stream (flate_hip_inflate_one_seek_index / _ranges), written ONCE:
// plain C++17 without HIP, compiled into the kernels (one_seek_kernels.hip), into the library's host code and into
// tests/host_model/seek_index_rule_model.cpp, which compares it with tests/seek_ref.py.
//
// n, unit_bit[0 .. n] and out_off[0 .. n] are flate_hip_inflate_one_index's; T = out_off[n].
//
// THE POINT RULE.  Unit k is a POINT iff k == 0 or out_off[k] / span > out_off[k - 1] / span (integer division):
// the first unit that starts in a new span of the output.  pstart(k) is the last point at or in front of k; a
// SEGMENT is a point and the units behind it up to the next point.
//
// THE INDEX, as 64-bit words: kSeekHeadWords of head (the kSeek* positions below), unit_bit[n + 1], out_off[n + 1],
// point_unit[n_points].  The windows: n_points - 1 blocks of kSeekWindow bytes, block p - 1 the output in front of
// unit point_unit[p].
#pragma once

#include <stdint.h>

#include "bgzf_range_rule.h"

namespace flate {

constexpr uint64_t kSeekMagic = 0x58444953454e4f46ull;  // "FONESIDX", little endian
constexpr uint64_t kSeekVersion = 1;
constexpr uint64_t kSeekSpanDefault = 1ull << 20;  // FLATE_HIP_SEEK_SPAN_DEFAULT
constexpr uint64_t kSeekSpanNone = ~0ull;          // FLATE_HIP_SEEK_SPAN_NONE
constexpr uint32_t kSeekWindow = 32768;
constexpr uint64_t kSeekUnitBitsMax = 8ull << 28;  // a unit's input spans at most 2^28 bytes ("one_unit_max")
// the head's words
constexpr uint32_t kSeekMagicAt = 0, kSeekVersionAt = 1, kSeekWrapAt = 2, kSeekInLenAt = 3, kSeekRawOffAt = 4,
                   kSeekRawEndAt = 5, kSeekTotalAt = 6, kSeekSpanAt = 7, kSeekUnitsAt = 8, kSeekPointsAt = 9,
                   kSeekWantAt = 10, kSeekIsizeAt = 11, kSeekRuleAt = 12, kSeekHeadWords = 16;  // (words 13 .. 15: 0)
// THE UNIT RULE the index was built with (word kSeekRuleAt; the option "one_stored_units" of the building context):
// units start at dynamic headers alone (0: every index from before the word existed), or at dynamic and stored headers.
// A read walks the units with THIS rule, whatever its own context's option says -- with another one TAIL would run on
// through a listed unit's end.
constexpr uint64_t kSeekRuleDynamic = 0, kSeekRuleStored = 1;

BGZF_HD uint64_t seek_span(uint64_t span) { return span ? span : kSeekSpanDefault; }

// THE POINT RULE for unit k of out_off (span >= 1: seek_span's result)
BGZF_HD bool seek_is_point(const uint64_t *out_off, uint32_t k, uint64_t span) {
  return k == 0u || out_off[k] / span > out_off[k - 1u] / span;
}

// the index of the last point at or in front of unit k in point_unit[0, n_points) (point_unit[0] == 0)
BGZF_HD uint32_t seek_point_of(const uint64_t *point_unit, uint32_t n_points, uint32_t k) {
  return bgzf_upper_bound(point_unit, n_points, k) - 1u;
}

BGZF_HD uint64_t seek_index_words(uint64_t n, uint64_t n_points) { return kSeekHeadWords + 2u * (n + 1u) + n_points; }
BGZF_HD uint64_t seek_windows_bytes(uint64_t n_points) { return n_points ? (n_points - 1u) * kSeekWindow : 0ull; }

// One range as the locate step leaves it: U[b, e), the first and the last unit with bytes inside it (kBgzfNoMember:
// the range is empty) and, for a non-empty range, seg = pstart(first): the units [seg, last] are decoded for it.
struct SeekLoc {
  uint64_t b, e;
  uint32_t first, last, seg;
};
BGZF_HD SeekLoc seek_locate(uint64_t begin, uint64_t end, const uint64_t *out_off, uint32_t n,
                            const uint64_t *point_unit, uint32_t n_points) {
  // (byte positions: bgzf_range_locate reads out_off alone)
  const BgzfRangeLoc L = bgzf_range_locate(kBgzfPosBytes, begin, end, out_off, out_off, n);
  SeekLoc r;
  r.b = L.b, r.e = L.e, r.first = L.first, r.last = L.last, r.seg = kBgzfNoMember;
  if (L.first != kBgzfNoMember) r.seg = (uint32_t)point_unit[seek_point_of(point_unit, n_points, L.first)];
  return r;
}

// Verdict 1 of flate_hip_inflate_one_ranges: the index describes SOME stream of in_len bytes in this container, and
// the arrays are what the counts imply.  Host, O(n); nothing outside index[0, index_words) is read.
inline bool seek_index_ok(const uint64_t *index, uint64_t index_words, uint64_t windows_bytes, uint32_t wrap,
                          uint64_t in_len) {
  if (!index || index_words < kSeekHeadWords) return false;
  if (index[kSeekMagicAt] != kSeekMagic || index[kSeekVersionAt] != kSeekVersion) return false;
  if (index[kSeekWrapAt] != wrap || index[kSeekInLenAt] != in_len) return false;
  const uint64_t n = index[kSeekUnitsAt], np = index[kSeekPointsAt], span = index[kSeekSpanAt];
  if (n < 1u || n >= 0xffffffffull || np < 1u || np > n || span < 1u) return false;
  if (index_words != seek_index_words(n, np) || windows_bytes != seek_windows_bytes(np)) return false;
  const uint64_t raw_off = index[kSeekRawOffAt], raw_end = index[kSeekRawEndAt], T = index[kSeekTotalAt];
  if (raw_off > raw_end || raw_end > in_len) return false;
  const uint64_t *unit_bit = index + kSeekHeadWords, *out_off = unit_bit + (n + 1u), *point_unit = out_off + (n + 1u);
  if (unit_bit[0] != 0u || out_off[0] != 0u || out_off[n] != T) return false;
  if (raw_end - raw_off > (~0ull >> 3) || unit_bit[n] > 8u * (raw_end - raw_off)) return false;
  for (uint64_t k = 0; k < n; ++k) {
    if (unit_bit[k + 1u] <= unit_bit[k] || unit_bit[k + 1u] - unit_bit[k] > kSeekUnitBitsMax) return false;
    if (out_off[k + 1u] < out_off[k]) return false;
  }
  uint64_t p = 0;
  for (uint64_t k = 0; k < n; ++k)
    if (seek_is_point(out_off, (uint32_t)k, span)) {
      if (p >= np || point_unit[p] != k) return false;
      ++p;
    }
  return p == np;
}

// ... and, for an index that passed seek_index_ok (the head is there): its unit rule is one this library walks by.
// Any other value fails like the cases above.
inline bool seek_index_rule_ok(const uint64_t *index) {
  return index[kSeekRuleAt] == kSeekRuleDynamic || index[kSeekRuleAt] == kSeekRuleStored;
}

}  // namespace flate
