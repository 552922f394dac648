// chain_rule.h -- what the discovery skeleton (chain_walk.h: BGZF members, gzip members, the units of one stream, a
// ZIP directory) decides without the device, written ONCE: plain C++17 without HIP, compiled into the kernels, into the
// library's host code and into tests/host_model/chain_walk_model.cpp, which holds it against a dictionary walk and
// against bgzf_serial_walk.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define CHAIN_HD __host__ __device__ inline
#else
#define CHAIN_HD inline
#endif

namespace flate {

// The tiles of the count and fill passes: one workgroup each, on the 16-byte grid of the buffer's ADDRESS (virtual
// position = file offset + A, A = address & 15, so that multiples of 16 are aligned addresses), one 16-byte chunk per
// thread and one more chunk of halo for a candidate's first bytes.
constexpr uint32_t kTileBytes = 4096;
constexpr uint32_t kTileHalo = 16;
constexpr uint32_t kTileChunks = kTileBytes / 16;  // 256: one per thread

// the tiles that cover the file offsets [lo, lo + len) of a buffer with that A, the first one at (lo + A) & ~15
CHAIN_HD uint64_t chain_tiles(uint64_t A, uint64_t lo, uint64_t len) {
  return (lo + A + len - ((lo + A) & ~15ull) + kTileBytes - 1) / kTileBytes;
}

// THE SEARCH.  cand_off[0, n) rises strictly.  Returns the i in [lo, n) with cand_off[i] == want, or n: there is none.
// At most 32 steps; nothing outside cand_off[lo, n) is read.
CHAIN_HD uint32_t chain_find(const uint64_t *cand_off, uint32_t lo, uint32_t n, uint64_t want) {
  uint32_t hi = n;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (cand_off[mid] < want) lo = mid + 1u;
    else hi = mid;
  }
  return (lo < n && cand_off[lo] == want) ? lo : n;
}

// THE LINK RULE.  The nodes are the n candidates and two sinks: n, the terminal node, and n + 1, the dead node; both
// absorb.  Candidate c < n goes to the dead node when it is not alive (its decode failed), to the terminal node when
// it is the last (it ends where the file does), else to the candidate at `want`, where it ends -- which lies strictly
// above c, so nothing cycles -- or, when no candidate starts there, to the dead node.
CHAIN_HD uint32_t chain_next(const uint64_t *cand_off, uint32_t c, uint32_t n, bool alive, bool last, uint64_t want) {
  if (c >= n) return c;
  if (!alive) return n + 1u;
  if (last) return n;
  const uint32_t at = chain_find(cand_off, c + 1u, n, want);
  return at < n ? at : n + 1u;
}
// ... and where the chain starts: candidate 0 when it sits at offset (or bit) 0, else the dead node
CHAIN_HD uint32_t chain_first(const uint64_t *cand_off, uint32_t n) { return (n && cand_off[0] == 0ull) ? 0u : n + 1u; }

}  // namespace flate
