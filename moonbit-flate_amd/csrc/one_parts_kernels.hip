// one_parts_kernels.hip -- ONE long stream read in PARTS (flate_hip_one_reader_*; flate_kernels.h: OnePartState,
// OnePartParams; the rule: one_parts_rule.h).  A call runs flate_hip_inflate_one's discovery and rounds over one part of
// the stream; what is the parts' own stands here: FIND's builds whose chain starts at the carried bit b0
// (one_find_kernel.inc says why they have a file of their own), and five small kernels around the unchanged PROBE,
// TAIL, COMPOSE, RESOLVE and DECODE.  No kernel waits for another workgroup; the only loop is the header's walk in
// one_part_init_kernel: one thread, bounded by the part's length (a FNAME without its NUL is walked to the part's end,
// as frame_parse_kernel walks it in the whole call).
#include <hip/hip_runtime.h>

#include "chain_walk.h"
#include "deflate_block_rule.h"
#include "flate_hip.h"
#include "one_parts_rule.h"

namespace flate {

#include "one_find_kernel.inc"

// the two unit rules, the root at bit b0
template __global__ void one_count_kernel<false, true>(OneParams P);
template __global__ void one_fill_kernel<false, true>(OneParams P);
template __global__ void one_count_kernel<true, true>(OneParams P);
template __global__ void one_fill_kernel<true, true>(OneParams P);

// One thread: the part's words.  bad: the rule's three answers (0 good, 1 bad, 2 "refused only because the part ends
// here"); anything but 0 leaves FIND no candidate, as a bad header does in the whole call.  Every read is below in_len.
__global__ void one_part_init_kernel(FrameOne *one, const uint8_t *in, uint64_t in_len, uint32_t wrap, uint32_t first,
                                     uint32_t final_in, uint32_t b0) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const OnePartFrame f = one_parts_frame(wrap, first != 0u, final_in != 0u, in, in_len);
  FrameOne o{};
  o.in_off[1] = in_len;
  o.pay_off[0] = f.raw_off;
  o.pay_off[1] = in_len;
  o.pay_end = f.raw_end;
  o.bad = f.hdr;
  o.dict_used = FLATE_HIP_NO_DICT;
  o.b0 = b0 & 7u;
  *one = o;
}

// One thread per node, as one_link_kernel; the chain starts at candidate 0, which FIND's PARTS build has put at bit b0.
__global__ __launch_bounds__(256) void one_part_link_kernel(OneParams P) {
  const uint32_t n = P.C.cap;
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  OneProbe pr{};
  if (c < n) pr = P.probe[c];
  chain_link(P.C, n, c, c < n && pr.status == 0, pr.final_block != 0u, pr.end_bit);
  if (c == 0) {
    P.C.member_off[0] = n ? P.C.cand_off[0] : 0ull;
    P.C.path[0] = n ? 0u : n + 1u;
  }
}

// One thread per entry of out_off (n of them).
__global__ __launch_bounds__(256) void one_part_hist_kernel(const uint64_t *out_off, uint64_t *tail_off, uint32_t n,
                                                            uint64_t hist_base) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k < n) tail_off[k] = out_off[k] + hist_base;
}

// One thread, behind the rounds (and the part's checksum, which the host has pointed at st->sums[1]).
__global__ void one_part_carry_kernel(OnePartParams Q, OneDecParams D) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  OnePartState *st = Q.st;
  OneDecHead r = *D.dh;
  const uint32_t fb = r.first_bad;
  r.out_len = Q.total;
  r.status = 0;
  r.err_off = -1;
  if (r.decode_bad != 0xffffffffu) {
    r.status = FLATE_HIP_E_INTERNAL;
    r.out_len = 0;
  } else if (fb != 0xffffffffu) {
    r.status = D.status[fb];
    r.err_off = D.err_off[fb];
    r.out_len = D.out_off[fb] + D.produced[fb];
  } else if (Q.term_rc != 0) {
    r.status = Q.term_rc;
    r.err_off = Q.term_err_off;
  }
  st->res = r;
  st->trailer_bad = 0u;
  st->slot_off[0] = 0;
  st->slot_off[1] = Q.produced_before;
  st->slot_off[2] = Q.produced_before + Q.total;
  st->produced[0] = Q.produced_before;
  st->produced[1] = Q.total;
}

// One thread, behind the join (or, in a call that only judges a trailer it has waited for, alone).
__global__ void one_part_verdict_kernel(OnePartParams Q) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  OnePartState *st = Q.st;
  if (st->res.status != 0) return;
  if (Q.wrap != FLATE_HIP_WRAP_RAW && Q.total != 0) st->sums[0] = Q.produced_before ? st->joined : st->sums[1];
  if (!Q.trailer || Q.wrap == FLATE_HIP_WRAP_RAW) return;
  const uint8_t *t = Q.trailer;
  uint32_t want, isize_off = 0;
  if (Q.wrap == FLATE_HIP_WRAP_GZIP) {
    want = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    const uint32_t isize = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
    isize_off = (uint32_t)(Q.produced_before + Q.total) ^ isize;
  } else {
    want = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3];
  }
  if (((st->sums[0] ^ want) | isize_off) != 0u) {
    st->res.status = FLATE_HIP_E_CORRUPT;
    st->res.err_off = (int64_t)Q.member_len;
    st->trailer_bad = 1u;
  }
}

}  // namespace flate
