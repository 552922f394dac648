// inflate_route.h -- which decoder a decode call runs, in which build and how it is launched (plain C++17, no HIP:
// tests/test_inflate_route.py compiles it on the CPU).  The kernels behind a route: launch_decoders, flate_api_inflate.hip.
#pragma once

#include <stdint.h>

namespace flate {

// flate_hip_set_option "inflate_*" (flate_hip_ctx::inflate)
struct InflateOpts {
  int lanes = 0;  // streams per wavefront of the lane-per-stream decoder: 0 = by batch size, or 16/32/64
  int row = 8;    // dwords of a lane's output row in the 64-lane form (0 = stores go straight to memory, 8, 16)
  // batches at least this large use the lane-per-stream inflater: it takes ~30 ms for 64 KiB
  // streams whatever the batch size, the wave-per-stream one ~13 ms per 1024 streams (measured:
  // tools/inflate_crossover.py)
  uint32_t simt_min = 2049;
  // the speculative wave-per-stream decoder (inflate_spec_kernel): 0 = never, 1 = for batches below
  // spec_max streams (where it beats both other decoders), 2 = always (tests)
  int spec = 1;
  int spec_shape = 0;  // 0 = by batch size, 1 / 2 = always the small-batch / large-batch build (tests, tuning)
  uint32_t spec_max = 45056;  // measured (tools/inflate_crossover.py, ms per batch of 64 KiB text streams,
                              // sub-block decoder against lane per stream; profiles/r04/inflate_crossover.txt):
                              // 8192: 6.7 / 29.3; 16384: 13.1 / 30.8; 32768: 26.0 / 32.4; 40960: 32.4 / 33.7;
                              // 49152: 38.8 / 35.3; 65536: 51.6 / 39.3 -- the lane-per-stream decoder wins
                              // from ~44 k streams on (round 3, with four of its wavefronts per CU: ~37 k)
};

enum InflateDecoder : int {
  kDecodeWave = 0,  // one wavefront per stream, scalar walk (inflate_kernel)
  kDecodeSimt = 1,  // one lane per stream (inflate_simt_kernel)
  kDecodeSpec = 2,  // one wavefront per stream, 64 sub-blocks at once (inflate_spec_kernel)
};

struct InflateRoute {
  int decoder;
  int shape;   // kDecodeSpec: 1 = the small-batch build, 2 = the large-batch build; else 0
  int lanes;   // kDecodeSimt: streams per wavefront (16 / 32 / 64); else 0
  int row;     // kDecodeSimt: dwords of the output row (0 / 8 / 16); else 0
  uint32_t blocks_per_launch;  // workgroups of a launch (the last launch of several may have fewer)
  uint32_t launches;
};

// the largest off[i + 1] - off[i]: one entry at a decoder's limit moves the whole batch
inline uint64_t longest_entry(const uint64_t *off, uint32_t n) {
  uint64_t longest = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (off[i + 1] - off[i] > longest) longest = off[i + 1] - off[i];
  return longest;
}

// ... of entries that end at end[i] (members that are not consecutive: InfParams::in_end)
inline uint64_t longest_entry(const uint64_t *off, const uint64_t *end, uint32_t n) {
  if (!end) return longest_entry(off, n);
  uint64_t longest = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (end[i] - off[i] > longest) longest = end[i] - off[i];
  return longest;
}

// longest: longest_entry of the call's in_off -- bytes of a stream, or, spliced, bits of a piece.
// size_only: FLATE_HIP_SIZE_ONLY was asked for (it holds for independent streams only).
inline InflateRoute inflate_route(const InflateOpts &o, uint32_t num_cus, uint32_t n, uint64_t longest, bool spliced,
                                  bool size_only) {
  size_only = size_only && !spliced;
  // large batches: one lane per stream (64 streams per wavefront); small ones: one wavefront per stream
  // (its bit positions are 32-bit: every compressed stream must be < 256 MiB)
  // (size-only passes never use the lane-per-stream decoder: it reads its history back from the
  // output it has written)
  const bool simt = (spliced || n >= o.simt_min) && !size_only && (spliced || longest < (1ull << 28));
  // (a size-only pass needs token lengths only: the sub-block decoder at any batch size, unless switched off)
  // 32-bit bit positions: a stream (a piece of a spliced stream: bit offsets then) below 256 MiB
  const bool spec = (o.spec == 2 || (o.spec == 1 && (size_only || n < o.spec_max))) &&
                    longest < (spliced ? (1ull << 31) : (1ull << 28));
  InflateRoute r{kDecodeWave, 0, 0, 0, n, 1};
  if (spec) {
    // (two builds of the same kernel: long token lists and a 16 KiB history ring while a SIMD holds
    // one wavefront, the small footprint beyond)
    r.decoder = kDecodeSpec;
    r.shape = o.spec_shape ? o.spec_shape : (n <= 4u * num_cus ? 1 : 2);
  } else if (simt) {
    r.decoder = kDecodeSimt;
    // (measured, same file: 16 lanes per wavefront up to ~20 k streams, 32 up to ~36 k, 64 beyond)
    r.lanes = o.lanes ? o.lanes : (n >= 144u * num_cus ? 64 : (n >= 80u * num_cus ? 32 : 16));
    // (the output row -- a lane's output collected in registers and stored as whole aligned pieces -- pays
    // where the chip is full of lanes: the 64-lane form only)
    r.row = r.lanes == 64 && (o.row == 8 || o.row == 16) ? o.row : 0;
    const uint32_t sblocks = (n + (uint32_t)r.lanes - 1) / (uint32_t)r.lanes;
    // A CU holds eight of these wavefronts (320 B of LDS per lane): a batch of more blocks than
    // that runs in ROUNDS, and a lane's rate depends little on how full the chip is -- so the rounds
    // are made equal (196608 streams: two launches of 98304 = 94 ms, against 60 + 47 for a full
    // round and a third of one).
    const uint32_t slots = 8u * num_cus;
    const uint32_t rounds = (sblocks + slots - 1) / slots;
    r.blocks_per_launch = (sblocks + rounds - 1) / (rounds ? rounds : 1u);
    r.launches = r.blocks_per_launch ? (sblocks + r.blocks_per_launch - 1) / r.blocks_per_launch : 0u;
  }
  return r;
}

// flate_hip_inflate_one: a round of n units of ONE stream -- spliced pieces (bit offsets) that each start from their
// own 32 KiB of resolved history (dictionaries).  Always the lane-per-stream decoder in its dictionary build: it is
// the one that ends a piece at the next piece's bit (InfParams::closed covers the round's last) and that takes a
// piece's history from the dictionary tail; lanes, row and launches as for any spliced call.
inline InflateRoute inflate_route_units(const InflateOpts &o, uint32_t num_cus, uint32_t n) {
  InflateOpts s = o;
  s.spec = 0;
  return inflate_route(s, num_cus, n, 0, true, false);
}

}  // namespace flate
