// chain_walk.h -- the skeleton the four discoveries share (BGZF members: bgzf_kernels.hip, gzip members:
// gzip_kernels.hip, the units of one stream: one_kernels.hip, a ZIP directory: zip_kernels.hip), device only, over
// ChainParams (flate_kernels.h).  A format brings its offset test, what a hit stores, and where a candidate ends; the
// decisions that need no device are chain_rule.h.  The contract of the tile functions:
//   - the workgroup is one-dimensional with exactly 256 threads, and every thread makes the call in uniform control
//     flow (the functions use barriers; their early returns depend on nothing but blockIdx and memory the launch
//     does not write);
//   - L is the kernel's `__shared__ TileLds`; every function ends behind a barrier or reads L no more;
//   - nothing outside in[0, in_len) is read.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "block_scan.h"
#include "chain_rule.h"
#include "flate_kernels.h"

namespace flate {

struct TileLds {  // a tile's bytes with their halo, and block_scan_excl's four words
  __attribute__((aligned(16))) uint8_t bytes[kTileBytes + kTileHalo];
  uint32_t wtot[4];
};

// A: where the buffer's first byte lies on the 16-byte grid
__device__ inline uint32_t tile_align(const uint8_t *in) { return (uint32_t)(reinterpret_cast<uintptr_t>(in) & 15u); }

// The bytes at the virtual positions [v0, v0 + kTileBytes + kTileHalo) into lds (16-byte aligned; v0 a multiple of
// 16): 16-byte loads, the chunks that cross either end of the file byte by byte; bytes outside the file read as zero.
// Ends behind a barrier.
__device__ inline void tile_load(const uint8_t *in, uint64_t in_len, uint8_t *lds, uint64_t v0, uint32_t A) {
  const uint64_t v_end = (uint64_t)A + in_len;
  for (uint32_t ch = threadIdx.x; ch <= kTileChunks; ch += 256u) {
    const uint64_t v = v0 + 16ull * ch;
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (v >= A && v + 16u <= v_end) {
      w = *reinterpret_cast<const uint4 *>(in + (v - A));
    } else if (v + 16u > A && v < v_end) {
      uint32_t d[4] = {0u, 0u, 0u, 0u};
      for (uint32_t b = 0; b < 16u; ++b) {
        const uint64_t vv = v + b;
        if (vv >= A && vv < v_end) d[b >> 2] |= (uint32_t)in[vv - A] << (8u * (b & 3u));
      }
      w = make_uint4(d[0], d[1], d[2], d[3]);
    }
    *reinterpret_cast<uint4 *>(lds + 16u * ch) = w;
  }
  __syncthreads();
}

// One tile pass, count form: the tile at virtual position v0 is loaded, mine = test(lds) is how many of this thread's
// offsets -- the 16 bytes from virtual position v0 + 16 * threadIdx.x, at lds + 16 * threadIdx.x -- hit, and the tile's
// sum goes to tile_cnt[blockIdx.x].
template <typename Test>
__device__ inline void tile_count(const ChainParams &C, TileLds &L, uint64_t v0, Test test) {
  tile_load(C.in, C.in_len, L.bytes, v0, tile_align(C.in));
  uint32_t sum = 0;
  (void)block_scan_excl<4, uint32_t>(test(L.bytes), L.wtot, &sum);
  if (threadIdx.x == 0) C.tile_cnt[blockIdx.x] = sum;
}

// The same pass, fill form, behind the scan, in two halves around the format's test (a callable that hands its hits
// on to the stores cost bgzf_fill_kernel scratch and zip_dir_fill_kernel LDS: profiles/chain_walk).  tile_fill_load: the tile is loaded and *first is the tile's
// first candidate; it returns false, to every thread and in front of every barrier, where nothing is to be stored:
// when the count does not fit the arrays (exact: when it is not C.cap, the count the host has read back and sized them
// from; else when it is above C.cap, and the host runs the pass again), and in a tile without hits.  tile_fill_at:
// the candidate this thread's first hit is, from how many hit; its hits go there and behind, the ones below C.cap.
__device__ inline bool tile_fill_load(const ChainParams &C, TileLds &L, uint64_t v0, bool exact, uint32_t *first) {
  const uint32_t n = C.head->n_cand;
  if (exact ? n != C.cap : n > C.cap) return false;  // (uniform)
  *first = C.tile_cnt[blockIdx.x];
  if (C.tile_cnt[blockIdx.x + 1] == *first) return false;  // (uniform: nothing in this tile)
  tile_load(C.in, C.in_len, L.bytes, v0, tile_align(C.in));
  return true;
}
__device__ inline uint32_t tile_fill_at(TileLds &L, uint32_t first, uint32_t mine) {
  uint32_t sum = 0;
  return first + block_scan_excl<4, uint32_t>(mine, L.wtot, &sum);
}
// ... and the stores of a format that tests bytes: bit b of hits = the byte offset b of this thread's 16 hit;
// store(at, b, k) receives the k-th of them
template <typename Store>
__device__ inline void tile_put16(uint32_t hits, uint32_t at, uint32_t cap, Store store) {
  uint32_t k = 0;
  for (uint32_t b = 0; b < 16u; ++b) {
    if (!((hits >> b) & 1u)) continue;
    if (at < cap) store(at, b, k);
    ++at, ++k;
  }
}

// One workgroup of 1024: tile_cnt[0, n_tiles] becomes its exclusive scan, saturating (above cap nothing downstream
// runs: the saturated value only has to stay above it), and the head is initialised: n_cand, and the verdict rc that
// stands until a finish kernel has found the chain's end.  wtot: 16 entries.
__device__ inline void tile_scan(const ChainParams &C, uint64_t *wtot, int32_t rc) {
  auto sat = [](uint64_t x) { return x > 0xffffffffull ? 0xffffffffu : (uint32_t)x; };
  const uint64_t n = scan_range<16, uint64_t>(
      C.n_tiles, wtot, [&](uint32_t i) { return (uint64_t)C.tile_cnt[i]; },
      [&](uint32_t i, uint64_t at, uint64_t) { C.tile_cnt[i] = sat(at); });
  if (threadIdx.x == 0) {
    C.tile_cnt[C.n_tiles] = sat(n);
    BgzfHead h;
    h.out_bytes = 0;
    h.err_off = 0;
    h.n_members = 0;
    h.rc = rc;
    h.eof_marker = 0;
    h.n_cand = sat(n);
    *C.head = h;
  }
}

// One thread per node c (n candidates and the two sinks): jump[0][c] = chain_next, path[0] = chain_first.  n is the
// candidate count the arrays were filled for; `want` is read for a candidate that is alive and not the last only.
__device__ inline void chain_link(const ChainParams &C, uint32_t n, uint32_t c, bool alive, bool last, uint64_t want) {
  if (c == 0) C.path[0] = chain_first(C.cand_off, n);
  if (c > n + 1u) return;
  C.jump[0][c] = chain_next(C.cand_off, c, n, alive, last, want);
}

}  // namespace flate
