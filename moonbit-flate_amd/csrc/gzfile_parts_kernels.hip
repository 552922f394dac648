// gzfile_parts_kernels.hip -- a gzip FILE of any members read in PARTS (flate_hip_gzfile_reader_*; flate_kernels.h:
// GzPartState, GzPartParams; the rule: gzfile_parts_rule.h).  A call runs flate_hip_gzfile_read's discovery and rounds
// over one part of the file; the chain is gzfile_kernels.hip's in the part's form, and what a part's DECODE needs
// stands here: the pieces of a round with the continued member's carried count and window (every form's: the whole
// file carries nothing), the trailers of the members that end among the delivered units, and the call's words.  No
// kernel waits for another workgroup; every loop is bounded by the segment count.
#include <hip/hip_runtime.h>

#include "chain_walk.h"
#include "flate_hip.h"
#include "gzfile_parts_rule.h"
#include "window_compose.h"

namespace flate {

// One thread per unit of the round (and one more): one_pieces_kernel's slots, with the history (never across a
// member), the seed and the end of a piece taken from the unit's member.  The units in front of the first header
// (u_member == 0xffffffff; the whole file has none) are the continued member's: hist bytes lie in front of them and
// their seed is R[0] -- the handle's window in the first round, the round driver's carry behind it.
__global__ __launch_bounds__(256) void gzfile_pieces_kernel(GzFileDecParams G, uint64_t hist) {
  const OneDecParams &D = G.D;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > D.count) return;
  const uint32_t u = D.u0 + i, fb = D.dh->first_bad;
  uint64_t limit = D.total;
  if (fb != 0xffffffffu) limit = D.out_off[fb] + D.produced[fb];
  if (limit > D.total) limit = D.total;
  uint64_t at = u > fb ? limit : D.out_off[u];  // (out_off is defined up to the first failing unit)
  if (at > limit) at = limit;
  D.p_out_off[i] = at;
  if (i == D.count) return;
  const uint32_t m = G.P.u_member[u];
  uint32_t f = 0u;    // its member's first unit in the part
  uint64_t rel = at + hist;
  if (m != 0xffffffffu) {
    f = (uint32_t)G.P.member_unit[m];
    rel = at > D.out_off[f] ? at - D.out_off[f] : 0ull;  // (a member behind the failure: an empty slot)
  }
  const uint32_t dict_len = rel < (uint64_t)kWinEntries ? (uint32_t)rel : kWinEntries;
  D.p_dict_len[i] = dict_len;
  D.p_dict_at[i] = (uint64_t)(i + 1u) * kWinEntries - dict_len;  // the tail of R[i]; R[i + 1] follows it
  G.seed[i] = f > D.u0 ? f - D.u0 : 0u;  // (a member that began in front of the round continues from R[0])
  G.p_bit_off[i] = D.unit_bit[u];
  // a member's last unit runs to BFINAL, and so does the unit the chain broke in
  G.p_bit_end[i] = (u >= G.n_good || G.P.u_final[u]) ? ~0ull : D.unit_bit[u + 1u];
}

// the sum of segment i's member up to the end of its bytes of this call
__device__ inline uint32_t gz_part_sum(const GzPartParams &Q, uint32_t i) {
  const GzPartSeg g = Q.segs[i];
  const bool bytes = g.out_end > g.out_begin;
  if (i == 0u && Q.sum0_mode == 1u) return Q.sums[0];
  if (i == 0u && Q.sum0_mode == 2u) return Q.st->joined;
  return bytes ? Q.sums[1u + i] : 0u;  // (the CRC-32 of nothing)
}

// One thread per member that ends among the delivered units, behind the checksums and the join.  A member is judged
// when every unit of it decoded: its last unit lies in front of the first failing one.
__global__ __launch_bounds__(256) void gzfile_part_trailer_kernel(GzPartParams Q, OneDecParams D) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= Q.n_end) return;
  if (D.dh->decode_bad != 0xffffffffu) return;
  const GzPartSeg g = Q.segs[i];
  if (g.last_unit >= D.dh->first_bad) return;
  const uint8_t *t = Q.in + g.trailer_at;
  const uint32_t want = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
  const uint32_t isize = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
  if (gz_part_sum(Q, i) != want || (uint32_t)g.size != isize) atomicMin(&Q.st->res.bad_trailer, i);
}

// One thread, behind the trailers.  The verdict in FILE order: a disagreement of the two decodes; else the first wrong
// trailer (its member lies in front of every failing unit: it was judged); else the first failing unit's verdict; else
// the chain's.  A call without a failure leaves the unfinished member's sum in the handle.
__global__ void gzfile_part_carry_kernel(GzPartParams Q, OneDecParams D) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  GzPartState *st = Q.st;
  GzFileVerdict v = st->res;  // (bad_trailer: the host's fill, then the ordered min)
  const uint32_t fb = D.dh->first_bad;
  v.out_len = Q.total;
  v.status = 0;
  v.bad_member = 0xffffffffu;
  v.err_off = -1;
  v.stream_err_off = -1;
  v.n_members = Q.n_end;
  v.n_units = Q.n_del;
  v.pad = 0;
  if (D.dh->decode_bad != 0xffffffffu) {
    v.status = FLATE_HIP_E_INTERNAL;
    v.out_len = 0;
    v.n_members = 0;
    v.n_units = 0;
  } else if (v.bad_trailer != 0xffffffffu) {
    const GzPartSeg g = Q.segs[v.bad_trailer];
    v.status = FLATE_HIP_E_CORRUPT;
    v.out_len = g.out_end;  // up to and including the member's last byte, and nothing behind it
    v.n_members = v.bad_trailer;
    v.n_units = g.last_unit + 1u;
  } else if (fb != 0xffffffffu) {
    v.status = D.status[fb];
    v.err_off = D.err_off[fb];
    v.bad_member = fb;
    v.out_len = D.out_off[fb] + D.produced[fb];
    v.n_units = fb;
    uint32_t whole = 0;
    while (whole < Q.n_end && Q.segs[whole].last_unit < fb) ++whole;
    v.n_members = whole;
  } else if (Q.term_rc != 0) {
    v.status = Q.term_rc;
    v.err_off = Q.term_err_off;
  } else {
    st->sum = Q.keep_sum ? gz_part_sum(Q, Q.n_segs - 1u) : 0u;
  }
  st->res = v;
}

}  // namespace flate
