// seek_pack_rule.h -- the PACKED windows of the seek index of ONE long stream (flate_hip_seek_windows_pack / _unpack,
// flate_hip_inflate_one_ranges_packed), written ONCE: plain C++17 without HIP, compiled into the kernels
// (seek_pack_mark_kernel.inc, seek_pack_kernels.hip), into the library's host code and into
// tests/host_model/seek_pack_rule_model.cpp, which compares it with tests/seek_pack_ref.py.
//
// The seek index (seek_index_rule.h) keeps, for every point p >= 1, block p - 1: the kSeekWindow bytes of output in
// front of P0 = out_off[point_unit[p]].  Window offset j of that block is output position P0 - kSeekWindow + j.
//
// THE KEEP RULE.  The point's segment is the output [P0, P1), P1 the next point's offset (or T).  A byte of the block
// is NEEDED iff some copy (q, len, dist) of the segment with q in [P0, min(P1, P0 + kSeekWindow)) has a source byte a
// in [q - dist, q - dist + len) with a < P0.  Later copies cannot reach the block (dist <= kSeekWindow); copies of
// copies are covered, because the first copy was counted where it happened.  A SPARSE block has every byte that is not
// needed set to zero.
//
// THE EMPTY-BLOCK RULE.  A block all of whose bytes are zero (after sparsifying, or as it came) is stored as NO bytes:
// off[b + 1] == off[b]; it is read back by zero fill without a decode.  Every other block is one raw DEFLATE stream:
// what flate_hip_deflate_fast_batch writes under flags 0 for its kSeekWindow bytes.
//
// THE PACK INDEX, as 64-bit words: kSeekPackHeadWords of head (the kSeekPack* positions below), then off[n_blocks + 1],
// byte offsets into `packed`, off[0] == 0, non-decreasing, off[n_blocks] == packed_bytes.
#pragma once

#include <stdint.h>

#include "seek_index_rule.h"

namespace flate {

constexpr uint64_t kSeekPackMagic = 0x4b505753454e4f46ull;  // "FONESWPK", little endian
constexpr uint64_t kSeekPackVersion = 1;
constexpr uint32_t kSeekPackCompress = 1u, kSeekPackSparse = 2u;  // FLATE_HIP_SEEK_PACK_COMPRESS / _SPARSE
// the head's words
constexpr uint32_t kSeekPackMagicAt = 0, kSeekPackVersionAt = 1, kSeekPackModeAt = 2, kSeekPackBlocksAt = 3,
                   kSeekPackBytesAt = 4, kSeekPackKeptAt = 5, kSeekPackBindAt = 6, kSeekPackBindWords = 5,
                   kSeekPackHeadWords = 16;  // (words 11 .. 15: 0)
// THE BINDING to the seek index the windows belong to: these words of its head, in this order
constexpr uint32_t kSeekPackBindOf[kSeekPackBindWords] = {kSeekInLenAt, kSeekTotalAt, kSeekSpanAt, kSeekUnitsAt, kSeekRuleAt};

BGZF_HD bool seek_pack_mode_ok(uint32_t mode) {
  return mode == kSeekPackCompress || mode == (kSeekPackCompress | kSeekPackSparse);
}
BGZF_HD uint64_t seek_pack_words(uint64_t n_blocks) { return kSeekPackHeadWords + n_blocks + 1u; }

// THE KEEP RULE for one copy: the half-open interval [lo, hi) of window offsets in [0, kSeekWindow] that the copy of
// len bytes at output position q with distance dist keeps of the block in front of P0; lo == hi == 0: none.  Empty for
// q - dist >= P0 and clipped at P0: an overlapping copy (dist < len) that starts in front of P0 keeps only its source
// bytes in front of P0.  Positions in front of the stream's first byte (P0 < kSeekWindow) are never kept -- a good
// stream has no such copy; the clip is for safety.  A q outside [P0, P0 + kSeekWindow), a dist outside [1, kSeekWindow]
// or len == 0 keep nothing.
struct SeekKeep {
  uint32_t lo, hi;
};
BGZF_HD SeekKeep seek_pack_keep(uint64_t q, uint32_t len, uint32_t dist, uint64_t P0) {
  SeekKeep none;
  none.lo = none.hi = 0u;
  if (q < P0 || q - P0 >= kSeekWindow || dist < 1u || dist > kSeekWindow || len == 0u) return none;
  const int64_t s = (int64_t)(q - P0) - (int64_t)dist;  // the first source byte, counted from P0
  if (s >= 0) return none;
  int64_t e = s + (int64_t)len;
  if (e > 0) e = 0;
  int64_t lo = s + (int64_t)kSeekWindow, hi = e + (int64_t)kSeekWindow;
  const int64_t front = P0 < kSeekWindow ? (int64_t)kSeekWindow - (int64_t)P0 : 0;  // window offset of the stream's byte 0
  if (lo < front) lo = front;
  if (lo >= hi) return none;
  SeekKeep k;
  k.lo = (uint32_t)lo, k.hi = (uint32_t)hi;
  return k;
}

// The pack index by itself: host, O(n_blocks); nothing outside pack_index[0, pack_words) is read.
inline bool seek_pack_self_ok(const uint64_t *pack_index, uint64_t pack_words, uint64_t packed_bytes) {
  if (!pack_index || pack_words < kSeekPackHeadWords + 1u) return false;
  if (pack_index[kSeekPackMagicAt] != kSeekPackMagic || pack_index[kSeekPackVersionAt] != kSeekPackVersion) return false;
  const uint64_t mode = pack_index[kSeekPackModeAt], nb = pack_index[kSeekPackBlocksAt];
  if (mode > 3u || !seek_pack_mode_ok((uint32_t)mode)) return false;
  if (nb >= 0xffffffffull || pack_words != seek_pack_words(nb)) return false;
  if (pack_index[kSeekPackBytesAt] != packed_bytes) return false;
  const uint64_t whole = nb * kSeekWindow, kept = pack_index[kSeekPackKeptAt];
  if ((mode & kSeekPackSparse) ? kept > whole : kept != whole) return false;
  for (uint32_t k = kSeekPackBindAt + kSeekPackBindWords; k < kSeekPackHeadWords; ++k)
    if (pack_index[k] != 0u) return false;
  const uint64_t *off = pack_index + kSeekPackHeadWords;
  if (off[0] != 0u || off[nb] != packed_bytes) return false;
  for (uint64_t b = 0; b < nb; ++b)
    if (off[b + 1u] < off[b]) return false;
  return true;
}

// ... and as the packed windows of `index`, a seek index that passed seek_index_ok (its head is there): the counterpart
// of seek_index_ok for (pack_index, packed) in the place of `windows`.
inline bool seek_pack_ok(const uint64_t *pack_index, uint64_t pack_words, uint64_t packed_bytes, const uint64_t *index) {
  if (!index || !seek_pack_self_ok(pack_index, pack_words, packed_bytes)) return false;
  if (pack_index[kSeekPackBlocksAt] + 1u != index[kSeekPointsAt]) return false;
  for (uint32_t k = 0; k < kSeekPackBindWords; ++k)
    if (pack_index[kSeekPackBindAt + k] != index[kSeekPackBindOf[k]]) return false;
  return true;
}

// the head of the pack index of `index` (the caller fills off[] behind it)
inline void seek_pack_head(uint64_t *pack_index, const uint64_t *index, uint32_t mode, uint64_t packed_bytes, uint64_t kept_bytes) {
  for (uint32_t k = 0; k < kSeekPackHeadWords; ++k) pack_index[k] = 0;
  pack_index[kSeekPackMagicAt] = kSeekPackMagic;
  pack_index[kSeekPackVersionAt] = kSeekPackVersion;
  pack_index[kSeekPackModeAt] = mode;
  pack_index[kSeekPackBlocksAt] = index[kSeekPointsAt] - 1u;
  pack_index[kSeekPackBytesAt] = packed_bytes;
  pack_index[kSeekPackKeptAt] = kept_bytes;
  for (uint32_t k = 0; k < kSeekPackBindWords; ++k) pack_index[kSeekPackBindAt + k] = index[kSeekPackBindOf[k]];
}

}  // namespace flate
