// checksum_join_model.cpp -- host model of checksum.hip's checksum_join_kernel (tests/test_checksum_join.py).
// The arithmetic is the kernel's own: moonbit-flate_amd/csrc/checksum_clip.h.  What is modelled here is only what
// surrounds it: the pieces' finished sums come from the caller (the kernel reads checksum_fold_kernel's), the bytes
// of the whole are added up first, and the pieces are then walked with a running prefix, one after another where the
// kernel walks them 1024 at a time.
#include <cstdint>

#include "checksum_clip.h"

using namespace flate;

// n pieces: piece i produced `produced[i]` bytes into a slot of `slot[i]` and has the sums adlers[i] / crcs[i] of the
// bytes it counts.  Returns 0, or 1: a piece's "bytes behind it" would wrap.
extern "C" int join_concat(const uint32_t *adlers, const uint32_t *crcs, const uint64_t *produced, const uint64_t *slot,
                           uint32_t n, uint32_t *adler, uint32_t *crc, uint64_t *total) {
  uint64_t n_bytes = 0;
  for (uint32_t i = 0; i < n; ++i) n_bytes += clip_to_slot(produced[i], slot[i]);
  const X2n T = make_x2n();
  uint32_t c = 0;
  uint64_t d1 = 0, d2 = 0, upto = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t len = clip_to_slot(produced[i], slot[i]);
    upto += len;
    if (upto > n_bytes) return 1;
    const uint64_t behind = n_bytes - upto;
    c ^= crc_concat_term(T, crcs[i], len, behind);
    const AdlerTerm t = adler_concat_term(adlers[i], len, behind);
    d1 = (d1 + t.d1) % kSumAdlerMod;
    d2 = (d2 + t.d2) % kSumAdlerMod;
  }
  *crc = c;
  *adler = adler_concat_finish(d1, d2, n_bytes);
  *total = n_bytes;
  return 0;
}
