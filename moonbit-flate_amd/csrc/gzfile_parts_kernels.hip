// gzfile_parts_kernels.hip -- a gzip FILE of any members read in PARTS (flate_hip_gzfile_reader_*; flate_kernels.h:
// GzPartState, GzPartParams; the rule: gzfile_parts_rule.h).  A call runs flate_hip_gzfile_read's discovery and rounds
// over one part of the file; every pass of those runs as it is, and what is the parts' own stands here: the member-wise
// kernels of gzfile_kernels.hip with the part's root, THE PARTS HOP, the continued member's carried count and window,
// and the trailers of the members that end among the delivered units.  No kernel waits for another workgroup; every
// loop is bounded by a header's length (the walks of gzip_header_len and one_parts_header, at most to the part's end),
// by the unit count or by 32 search steps.
#include <hip/hip_runtime.h>

#include "chain_walk.h"
#include "flate_hip.h"
#include "gzfile_parts_rule.h"
#include "window_compose.h"

namespace flate {

// One thread: the part's words.  The raw range is in[0, in_len - 8), as gzfile_init_kernel's.  bad: the root's verdict
// at a BOUNDARY (the rule's three answers); anything but 0 leaves FIND no candidate.  Every read is below in_len.
__global__ void gzfile_part_init_kernel(FrameOne *one, const uint8_t *in, uint64_t in_len, uint32_t inside, uint32_t b0) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  FrameOne o{};
  o.in_off[1] = in_len;
  o.pay_off[1] = in_len;
  o.pay_end = in_len >= kGzipTrailerLen ? in_len - kGzipTrailerLen : 0ull;
  o.dict_used = FLATE_HIP_NO_DICT;
  if (inside) {
    o.b0 = b0 & 7u;
  } else {
    uint64_t hl = 0;
    o.bad = gzfile_parts_root(in, in_len, &hl);
  }
  *one = o;
}

// One thread per node (n_a + n_b + 2 of them).
__global__ __launch_bounds__(256) void gzfile_part_link_kernel(GzFileParams P, uint32_t inside, uint32_t final_in) {
  const ChainParams &C = P.O.C;
  const uint32_t n = C.cap, na = P.n_a;
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c == 0) {
    // INSIDE: candidate 0, which FIND's PARTS build has put at bit b0; BOUNDARY: the member at offset 0
    if (inside) C.path[0] = na ? 0u : n + 1u;
    else C.path[0] = (P.n_b && P.hdr_off[0] == 0ull) ? na : n + 1u;
    OneHead h{};
    h.h.rc = FLATE_HIP_E_CORRUPT;
    h.h.n_cand = n;
    h.raw_len = P.O.one->pay_end;
    *P.O.head = h;
    GzFileHead g{};
    g.err_off = 0;
    g.stream_err_off = -1;
    g.no_header = 1u;
    g.pad[0] = kGzPartEndDead;
    *P.gh = g;
    C.member_off[0] = 0ull;
    P.u_start[0] = 0ull;
  }
  if (c > n + 1u) return;
  uint32_t next = c;  // (the sinks absorb)
  if (c < n) {
    const OneProbe pr = P.O.probe[c];
    next = n + 1u;
    if (pr.status != 0) {
    } else if (!pr.final_block) {
      const uint32_t at = chain_find(C.cand_off, 0u, na, pr.end_bit);
      if (at < na) next = at;
    } else {
      const GzHop hop = gzfile_parts_hop(C.in, C.in_len, pr.end_bit, final_in != 0u);
      if (hop.kind == kGzHopEnd || hop.kind == kGzHopStop) {
        next = n;
      } else if (hop.kind == kGzHopNext) {
        const uint32_t at = chain_find(P.hdr_off, 0u, P.n_b, hop.e);
        if (at < P.n_b) next = na + at;
      }
    }
  }
  C.jump[0][c] = next;
}

__global__ __launch_bounds__(256) void gzfile_part_finish_kernel(GzFileParams P, uint32_t final_in) {
  const ChainParams &C = P.O.C;
  const uint32_t n = C.cap;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r + 1u >= C.path_len) return;  // (the last entry is a sink: see below)
  const uint32_t c = C.path[r];
  if (c >= n) return;
  BgzfHead *h = C.head;
  const OneProbe pr = P.O.probe[c];
  C.member_off[r] = C.cand_off[c];
  P.u_start[r] = c >= P.n_a ? P.hdr_off[c - P.n_a] + 1u : 0ull;
  if (pr.status != 0) {  // the decode ends IN this unit: one thread gets here, or one gets below
    const bool deliver = pr.status != FLATE_HIP_E_TOO_LARGE;
    P.O.head->fail_out = deliver ? pr.out : 0ull;
    P.O.head->fail_unit = deliver ? 1u : 0u;
    h->n_members = r;
    h->rc = pr.status;
    h->err_off = pr.err_off;
    P.gh->no_header = 0u;
    return;
  }
  P.O.usize[r] = pr.out;
  P.u_final[r] = pr.final_block;
  // (the chain holds at most n nodes and path_len >= n + 2: r + 1 is inside the path)
  const uint32_t succ = C.path[r + 1u];
  if (succ < n) return;
  h->n_members = r + 1u;  // this is the last good unit
  C.member_off[r + 1u] = pr.end_bit;
  P.u_start[r + 1u] = 0ull;
  P.gh->no_header = 0u;
  if (pr.final_block) {  // how the chain ended: the hop again
    const GzHop hop = gzfile_parts_hop(C.in, C.in_len, pr.end_bit, final_in != 0u);
    if (succ == n) {
      h->rc = 0;
      h->err_off = -1;
      P.gh->pad[0] = hop.kind == kGzHopEnd ? kGzPartEndFile : kGzPartEndStop;
      P.gh->err_off = (int64_t)hop.e;
    } else {  // no member can start behind this one's trailer
      h->rc = FLATE_HIP_E_CORRUPT;
      h->err_off = (int64_t)hop.e;
      P.gh->no_header = 1u;
    }
  } else {  // a header of a unit-starting type that is no candidate: the tail probe reads it as the serial decoder
    P.O.head->tail_bit = pr.end_bit;
    P.O.head->tail = 1u;
  }
}

// One thread per unit (and the one behind the good ones), behind gzfile_members_kernel.  hist: what the continued member
// produced before the part, as far as the distance rule can see it (it saturates at the window).
__global__ __launch_bounds__(256) void gzfile_part_rel_kernel(GzFileParams P, uint64_t hist) {
  const ChainParams &C = P.O.C;
  const uint32_t nu = C.head->n_members;
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k > nu) return;
  const uint32_t m = P.u_member[k];
  P.rel_off[k] = m == 0xffffffffu ? hist + C.out_off[k] : C.out_off[k] - C.out_off[P.member_unit[m]];
}

// One thread per unit of the round (and one more): gzfile_pieces_kernel, with the continued member's units seeded by
// R[0] -- the handle's window in the first round, the round driver's carry behind it.
__global__ __launch_bounds__(256) void gzfile_part_pieces_kernel(GzFileDecParams G, uint64_t hist) {
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
