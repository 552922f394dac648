// seek_pack_mark_kernel.inc -- part of inflate_kernels.hip, behind one_probe_kernel.inc (it uses the shared reader:
// read_block_header, read_stored_len, read_tables, read_copy, huff_sym, and WalkShared).  MARK + SPARSIFY of
// flate_hip_seek_windows_pack (seek_pack_rule.h: THE KEEP RULE), one wavefront per block of the seek index's windows.
//
// MARK is a sibling of one_walk, not a further build of it: it walks from the bit of point p = block + 1 through block
// AND unit headers alike (the unit rule of the index does not matter), stops once kSeekWindow bytes of output have
// passed or at the segment's end bit, keeps no window and stores nothing of the stream's output.  Every copy whose
// source reaches in front of the point sets the bits of seek_pack_keep's interval in a 4 KiB mask in LDS.  A walk that
// fails, meets a distance in front of the stream's first byte, or leaves the segment anywhere but at its end bit with
// exactly the segment's bytes says that the stream is not the index's: status FLATE_HIP_E_CORRUPT, nothing written to
// the slot.  Every loop consumes input bits or ends: a walk is bounded by the raw stream's length.
// A segment whose first kSeekWindow bytes of output take more than 2^30 bytes of input (a flood of empty blocks) is
// refused as corrupt: the reader counts in 32 bits.
//
// SPARSIFY: the same wavefront reads the raw block (any alignment), zeroes what the mask does not keep, writes the 16
// byte pieces to slot `block` of the dense scratch and records "has a non-zero byte" and the kept count.
struct MarkShared {
  WalkShared<false> w;
  uint32_t mask[kSeekWindow / 32u];
  uint32_t any, kept;
};

__global__ __launch_bounds__(64) void seek_pack_mark_kernel(SeekMarkParams M) {
  __shared__ MarkShared sh;
  const int lane = threadIdx.x;
  const uint32_t blk = blockIdx.x;
  if (blk + 1u >= M.n_points) return;
  const uint32_t p = blk + 1u;
  const uint32_t u = (uint32_t)M.point_unit[p];
  const uint32_t u_end = p + 1u < M.n_points ? (uint32_t)M.point_unit[p + 1u] : M.n;
  const uint64_t P0 = M.out_off[u], seg_out = M.out_off[u_end] - P0;
  const uint64_t start = M.unit_bit[u], end_bit = M.unit_bit[u_end];  // (unit_bit[n]: behind the final block)
  // copies at q - P0 below this are marked; at or behind it the walk stops unless the whole segment is walked
  const uint64_t mark_end = seg_out < (uint64_t)kSeekWindow ? seg_out : (uint64_t)kSeekWindow;
  const bool whole = seg_out <= (uint64_t)kSeekWindow;

  for (uint32_t j = lane; j < kSeekWindow / 32u; j += 64) sh.mask[j] = 0u;
  if (lane == 0) sh.any = 0u, sh.kept = 0u;

  const uint64_t raw_off = M.one->pay_off[0], raw_end = M.one->pay_end;
  bool bad = M.one->bad != 0u || raw_off > raw_end || raw_end > M.in_len;
  const uint64_t raw_len = bad ? 0ull : raw_end - raw_off;
  const uint64_t base = start >> 3;
  const uint32_t k = (uint32_t)start & 7u;
  if (base >= raw_len) bad = true;
  bad = uni(bad ? 1u : 0u) != 0u;
  if (!bad) {
    const uint64_t left = raw_len - base;
    const uint8_t *in = M.in + raw_off + base;
    Bits b;
    b.in_len = (uint32_t)(left > (1ull << 30) ? (1ull << 30) : left);
    b.roff = k ? 1u : 0u;
    b.ipos = 0;
    b.sbase = 0;
    b.buf = 0;
    b.cnt = 0;
    b.avail = k ? 8 - (int)k : 0;
    uint64_t opos = 0;
    int err = 0;
    bool final_block = false, stop = false;
    auto step = [&]() {
      bits_pin(b);
      err = (int)uni((uint32_t)err);
      if (stage_low(b)) restage(b, sh.w.stage, in, lane);
    };
    auto bit_now = [&]() { return 8ull * (base + b.roff) - (uint64_t)b.avail; };
    restage(b, sh.w.stage, in, lane);  // (its barrier also publishes the cleared mask)
    b.buf >>= k;  // the bits in front of the point
    b.cnt -= (int)k;
    for (;;) {
      step();
      if (bit_now() >= end_bit) break;  // the segment's end (judged below)
      uint32_t typ;
      if ((err = read_block_header(b, sh.w.stage, final_block, typ))) break;
      if (typ == 0) {
        const int n = read_stored_len(b, in);
        if (n < 0) {
          err = n;
          break;
        }
        const uint32_t ip = b.roff, avail = b.in_len - ip;
        const uint32_t cnt = avail < (uint32_t)n ? avail : (uint32_t)n;
        opos += cnt;
        b.roff += cnt;
        if (cnt < (uint32_t)n) {
          err = E_EOF;
          break;
        }
        b.ipos = b.roff;
        b.buf = 0;
        b.cnt = 0;
        b.avail = 0;
        restage(b, sh.w.stage, in, lane);
      } else {
        int lit_min, lit_max, dist_min, dist_max, nlit;
        if ((err = read_tables(b, sh.w, typ, lane, step, lit_min, lit_max, dist_min, dist_max, nlit))) break;
        for (;;) {
          step();
          const int v = huff_sym(b, sh.w.lit, lit_min, lit_max, sh.w.stage, &err);
          if (v < 0 || v == 256) break;
          if (v < 256) {
            ++opos;
          } else {
            int length, dist;
            if ((err = read_copy(b, sh.w.dist, dist_min, dist_max, sh.w.stage, v, length, dist))) break;
            if ((uint64_t)dist > opos) {  // the source starts in front of the point
              if ((uint64_t)dist > opos + P0) {  // ... and in front of the stream
                err = E_CORRUPT;
                break;
              }
              if (opos < mark_end) {
                const SeekKeep keep = seek_pack_keep(P0 + opos, (uint32_t)length, (uint32_t)dist, P0);
                if (keep.hi > keep.lo) {  // at most 9 words of the mask: one per lane
                  const uint32_t w = (keep.lo >> 5) + (uint32_t)lane;
                  if (w <= ((keep.hi - 1u) >> 5)) {
                    const uint32_t lo = keep.lo > 32u * w ? keep.lo - 32u * w : 0u;
                    const uint32_t hi = keep.hi < 32u * w + 32u ? keep.hi - 32u * w : 32u;
                    const uint32_t bits = (hi >= 32u ? ~0u : (1u << hi) - 1u) & ~((1u << lo) - 1u);
                    atomicOr(&sh.mask[w], bits);
                  }
                }
              }
            }
            opos += (uint32_t)length;
          }
          if (!whole && opos >= (uint64_t)kSeekWindow) {  // 32 KiB of output have passed: no later copy reaches the block
            stop = true;
            break;
          }
        }
        if (err || stop) break;
      }
      if (!whole && opos >= (uint64_t)kSeekWindow) {
        stop = true;
        break;
      }
      if (final_block) break;
    }
    err = (int)uni((uint32_t)err);
    if (err)
      bad = true;
    else if (!stop)  // the walk ran to the segment's end: exactly its end bit, exactly its bytes
      bad = bit_now() != end_bit || opos != seg_out || final_block != (u_end == M.n);  // (the last one: BFINAL)
  }
  __syncthreads();
  if (!bad) {
    const uint8_t *src = M.windows + (uint64_t)blk * kSeekWindow;
    uint8_t *dst = M.dense + (uint64_t)blk * kSeekWindow;
    const bool aligned = ((uintptr_t)src & 3u) == 0u;
    uint32_t any = 0u, kept = 0u;
    for (uint32_t c = (uint32_t)lane; c < kSeekWindow / 16u; c += 64u) {
      const uint32_t m = (sh.mask[c >> 1] >> (16u * (c & 1u))) & 0xffffu;
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (m) {
        if (aligned) {
          const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src + 16u * c);
          for (uint32_t t = 0; t < 4u; ++t) w[t] = s32[t];
        } else {
          for (uint32_t t = 0; t < 16u; ++t) w[t >> 2] |= (uint32_t)src[16u * c + t] << (8u * (t & 3u));
        }
        for (uint32_t t = 0; t < 4u; ++t) {
          const uint32_t mm = (m >> (4u * t)) & 15u;  // one mask bit per byte -> 0xff per byte
          const uint32_t spread = ((mm & 1u) ? 0xffu : 0u) | ((mm & 2u) ? 0xff00u : 0u) | ((mm & 4u) ? 0xff0000u : 0u) |
                                  ((mm & 8u) ? 0xff000000u : 0u);
          w[t] &= spread;
          any |= w[t];
        }
        kept += (uint32_t)__popc(m);
      }
      *reinterpret_cast<uint4 *>(dst + 16u * c) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (any) atomicOr(&sh.any, 1u);
    atomicAdd(&sh.kept, kept);
  }
  __syncthreads();
  if (lane == 0) {
    SeekPackBlock r;
    r.nonzero = bad ? 0u : sh.any;
    r.kept = bad ? 0u : sh.kept;
    r.status = bad ? E_CORRUPT : 0;
    r.pad = 0u;
    M.blk[blk] = r;
  }
}
