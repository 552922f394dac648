// one_find_kernel.inc -- FIND of the block discovery (one_kernels.hip: one_count_kernel / one_fill_kernel), as templates
// on the unit rule.  Included inside namespace flate by the files that instantiate them: one_kernels.hip the build
// for dynamic headers alone (the default), one_stored_kernels.hip the one for dynamic and stored headers (option
// "one_stored_units"), one_parts_kernels.hip those of a stream read in parts, whose chain starts at a carried bit.
// A file of its own per build ON PURPOSE: how the compiler inlines the rule into a kernel depends on how many kernels
// of the same file call it, and the default build's instructions must not depend on the others' existence.  (The
// PARTS test is a template flag for the same reason: one_kernels.hip and one_stored_kernels.hip compile to what they
// were before it existed.)

namespace {

// this thread's 128 bit offsets: bit j of hits = a unit can start at bit (j & 7) of the byte at virtual position
// v0 + 16 * tid + (j >> 3).  Returns how many.  STORED (option "one_stored_units"): a stored header starts a unit too --
// the rule reads at most the 6 bytes from the bit's byte on, in LDS like the head test's; only its "four bytes inside
// the raw range" comparison sees the stream's end.  The dynamic-only build holds no trace of it.
// PARTS (a stream read in parts, one_parts_kernels.hip): the first unit starts at bit b0 = FrameOne::b0 of the raw
// range's first byte, not at bit 0.  That bit is a candidate whatever it holds, and the bits in front of it in that byte
// -- bits of the unit the last call delivered -- are none: the root stays candidate 0 and no decoy can stand in front
// of it.  The other builds hold no trace of it.
template <bool STORED, bool PARTS>
__device__ inline uint32_t test_bits(const OneParams &P, const uint8_t *lds, uint64_t v0, uint32_t A, uint32_t hits[4]) {
  hits[0] = hits[1] = hits[2] = hits[3] = 0u;
  const uint64_t raw_off = P.one->pay_off[0], raw_end = P.one->pay_end;
  const bool bad = P.one->bad != 0;
  const uint32_t at = 16u * threadIdx.x;
  uint32_t n = 0;
  for (uint32_t b = 0; b < 16u; ++b) {
    const uint64_t v = v0 + at + b;
    if (v < A) continue;
    const uint64_t p = v - A;
    if (bad || p < raw_off || p >= P.C.in_len) continue;
    uint32_t m = 0;
    if (p < raw_end) {
      const uint64_t end_bit = 8u * (raw_end - p);  // (the bytes the head test reads lie in LDS: see above)
      // the cheap rejections first: 13 bits of a 32-bit window (bits behind the stream's end fail in dblk_head_ok)
      const uint8_t *l = lds + at + b;
      const uint32_t w = l[0] | ((uint32_t)l[1] << 8) | ((uint32_t)l[2] << 16) | ((uint32_t)l[3] << 24);
      for (uint32_t k = 0; k < 8u; ++k)
        if (dblk_quick_ok(w >> k) && dblk_head_ok(l, end_bit, k) &&
            deflate_dyn_header_ok(P.C.in + raw_off, raw_end - raw_off, 8u * (p - raw_off) + k))
          m |= 1u << k;
      if constexpr (STORED)
        for (uint32_t k = 0; k < 8u; ++k)
          if (deflate_stored_header_ok(l, raw_end - p, k)) m |= 1u << k;
    }
    if (p == raw_off) {
      if constexpr (PARTS) m = (m | (1u << (P.one->b0 & 7u))) & (0xffu << (P.one->b0 & 7u)) & 0xffu;
      else m |= 1u;  // bit 0 starts the first unit
    }
    hits[b >> 2] |= m << (8u * (b & 3u));
    n += (uint32_t)__popc(m);
  }
  return n;
}

}  // namespace

template <bool STORED, bool PARTS>
__global__ __launch_bounds__(256) void one_count_kernel(OneParams P) {
  __shared__ TileLds L;
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // (chain_scan_kernel writes head->h, and nothing behind it)
    P.head->tail_bit = 0;
    P.head->tail = 0;
    P.head->prefix_bytes = 0;
    P.head->fail_out = 0;
    P.head->fail_unit = 0;
    P.head->pad = 0;
    P.head->bad = P.one->bad;
    P.head->raw_off = P.one->pay_off[0];
    P.head->raw_len = P.one->pay_end - P.one->pay_off[0];
  }
  const uint32_t A = tile_align(P.C.in);
  const uint64_t v0 = (uint64_t)blockIdx.x * kTileBytes;
  uint32_t hits[4];
  tile_count(P.C, L, v0, [&](const uint8_t *lds) { return test_bits<STORED, PARTS>(P, lds, v0, A, hits); });
}

template <bool STORED, bool PARTS>
__global__ __launch_bounds__(256) void one_fill_kernel(OneParams P) {
  __shared__ TileLds L;
  const uint32_t A = tile_align(P.C.in), cap = P.C.cap;
  const uint64_t v0 = (uint64_t)blockIdx.x * kTileBytes;
  uint32_t first, hits[4];
  if (!tile_fill_load(P.C, L, v0, true, &first)) return;
  uint32_t at = tile_fill_at(L, first, test_bits<STORED, PARTS>(P, L.bytes, v0, A, hits));
  const uint64_t raw_off = P.one->pay_off[0];
  for (uint32_t j = 0; j < 128u; ++j) {
    if (!((hits[j >> 5] >> (j & 31u)) & 1u)) continue;
    // (a hit lies at or above raw_off: test_bits)
    if (at < cap) P.C.cand_off[at] = 8u * (v0 + 16u * threadIdx.x + (j >> 3) - A - raw_off) + (j & 7u);
    ++at;
  }
}
