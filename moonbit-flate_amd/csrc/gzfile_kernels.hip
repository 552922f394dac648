// gzfile_kernels.hip -- a gzip FILE of any members, whole (flate_hip_gzfile_index / _read) or in PARTS
// (flate_hip_gzfile_reader_*): the units of all members as ONE chain over the bits of the file or the part, the members
// found from it, and the whole call's result words (flate_kernels.h: GzFileParams, GzFileMode, GzFileDecParams; the
// rules: gzfile_rule.h, gzfile_parts_rule.h, gzfile_parts_serial_rule.h).
//
// The skeleton is chain_walk.h's with two candidate lists in one node array.  The passes are the existing ones:
// one_count_kernel / one_fill_kernel (List A: every bit that passes the dynamic-header rule; the raw stream they are
// given is in[0, in_len - 8)), gzip_count_kernel / gzip_fill_kernel with no clip (List B: every byte that passes the
// gzip header rule), one_probe_kernel over all nodes, chain_round_kernel, one_out_scan_kernel and the tail probe.  What
// is this format's own (M: the form, which for the whole file is the part that is final and starts at a BOUNDARY):
//   gzfile_init_kernel     M; the one range: bits and error offsets are counted from the first byte; a part's root
//   gzfile_bits_kernel     a B node's bit: 8 * (header offset + header length)
//   gzfile_link_kernel     M; in front of a dynamic header: the A node at that bit; behind BFINAL: THE LINK into B
//   gzfile_finish_kernel   M; path rank r -> unit_bit[r], the unit's size, whether it starts and whether it ends a member;
//                          the thread at which the path meets a sink writes how the chain ended or asks for the tail probe
//   gzfile_members_kernel  the scan over the "starts a member" marks -> member_off, member_unit, u_member
//   gzfile_rel_kernel      M; rel_off, and for the whole file member_out and the verdict's member words
//   gzfile_trailer_kernel  the whole file, one thread per member: CRC-32 and ISIZE against its trailer, an ordered min
//   gzfile_verdict_kernel  the whole call's result words
// A unit ends strictly above its start and a hop lands above the trailer it skips, so nothing cycles.  No kernel waits
// for another workgroup; every loop is bounded by a header's length, by the unit count or by 32 search steps.
#include <hip/hip_runtime.h>

#include "chain_walk.h"
#include "flate_hip.h"
#include "gzfile_parts_serial_rule.h"
#include "window_compose.h"

namespace flate {

// One thread.  The raw range is in[0, in_len - 8): the last 8 bytes can only be a trailer.  A part takes b0 INSIDE, and
// at a BOUNDARY the root's verdict (the rule's three answers; anything but 0 leaves FIND no candidate) from in[0, in_len).
__global__ void gzfile_init_kernel(FrameOne *one, const uint8_t *in, uint64_t in_len, GzFileMode M, uint32_t b0) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  FrameOne o{};
  o.in_off[1] = in_len;
  o.pay_off[1] = in_len;
  o.pay_end = in_len >= kGzipTrailerLen ? in_len - kGzipTrailerLen : 0ull;
  o.dict_used = FLATE_HIP_NO_DICT;
  if (M.inside) {
    o.b0 = b0 & 7u;
  } else if (M.part) {
    uint64_t hl = 0;
    o.bad = gzfile_parts_root(in, in_len, &hl);
  }
  *one = o;
}

// One thread per B node.
__global__ __launch_bounds__(256) void gzfile_bits_kernel(GzFileParams P) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= P.n_b) return;
  // (never 0: the fill pass applied the same rule over the same range)
  P.O.C.cand_off[P.n_a + j] = gzfile_first_bit(P.O.C.in, P.O.C.in_len, P.hdr_off[j]);
}

// One thread per node (n_a + n_b + 2 of them).  THE LINK behind BFINAL is gzfile_parts_serial_hop: with no verdicts
// THE PARTS HOP, and that on a final part THE HOP.
__global__ __launch_bounds__(256) void gzfile_link_kernel(GzFileParams P, GzFileMode M) {
  const ChainParams &C = P.O.C;
  const uint32_t n = C.cap, na = P.n_a, nb = P.n_b;
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c == 0) {
    // INSIDE: candidate 0, which FIND's PARTS build has put at bit b0; BOUNDARY: the member at offset 0; until a finish
    // thread knows better: no member can start there
    if (M.inside) C.path[0] = na ? 0u : n + 1u;
    else C.path[0] = (nb && P.hdr_off[0] == 0ull) ? na : n + 1u;
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
      const GzHop hop = gzfile_parts_serial_hop(C.in, C.in_len, pr.end_bit, M.final_in != 0u, [&](uint64_t e) {
        if (!M.verdict) return kGzPartLong;
        const uint32_t at = chain_find(P.hdr_off, 0u, nb, e);
        return at < nb ? M.verdict[at] : kGzPartLong;
      });
      if (hop.kind == kGzHopEnd || hop.kind == kGzHopStop) {
        next = n;
      } else if (hop.kind == kGzHopNext) {
        const uint32_t at = chain_find(P.hdr_off, 0u, nb, hop.e);
        if (at < nb) next = na + at;
      }
    }
  }
  C.jump[0][c] = next;
}

__global__ __launch_bounds__(256) void gzfile_finish_kernel(GzFileParams P, GzFileMode M) {
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
  if (pr.final_block) {  // how the chain ended: the hop again (succ == n lies only behind a final block)
    const GzHop hop = gzfile_parts_hop(C.in, C.in_len, pr.end_bit, M.final_in != 0u);
    if (succ == n) {
      h->rc = 0;
      h->err_off = -1;
      // for gzfile_part_serial_stop_kernel and no one else; the whole file's rel kernel writes err_off over
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

// One workgroup, behind the out-scan: the scan over the marks of the good units and the one the chain broke in.
__global__ __launch_bounds__(1024) void gzfile_members_kernel(GzFileParams P) {
  __shared__ uint32_t wtot[16];
  const uint32_t hi = P.O.C.head->n_members + 1u;
  (void)scan_range<16, uint32_t>(
      hi, wtot, [&](uint32_t k) { return P.u_start[k] ? 1u : 0u; },
      [&](uint32_t k, uint32_t before, uint32_t v) {
        P.u_member[k] = before + v - 1u;  // (0xffffffff: in front of every member)
        if (v) {
          P.member_off[before] = P.u_start[k] - 1u;
          P.member_unit[before] = k;
        }
      });
}

// One thread per unit (and the one behind the good ones), behind gzfile_members_kernel and the tail probe.  A unit in
// front of every member is the continued member's and starts at M.hist (the whole file: only the unit behind no good
// one, at 0).  The member words are the whole file's: a reader's call counts its members on the host.
__global__ __launch_bounds__(256) void gzfile_rel_kernel(GzFileParams P, GzFileMode M) {
  const ChainParams &C = P.O.C;
  const uint32_t nu = C.head->n_members;
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k > nu) return;
  const uint32_t m = P.u_member[k];
  P.rel_off[k] = m == 0xffffffffu ? M.hist + C.out_off[k] : C.out_off[k] - C.out_off[P.member_unit[m]];
  if (M.part) return;
  if (P.u_start[k]) P.member_out[m] = C.out_off[k];
  if (k != nu) return;
  // the verdict's member words; m = the member of the unit the chain broke in, or the last whole member
  GzFileHead *g = P.gh;
  const int32_t rc = C.head->rc;
  const uint32_t whole = m + 1u;
  if (rc == 0 || g->no_header) {  // every member in front is whole
    g->n_members = whole;
    P.member_off[whole] = rc == 0 ? C.in_len : (uint64_t)C.head->err_off;
    P.member_unit[whole] = nu;
    P.member_out[whole] = C.out_off[nu];
    g->err_off = rc == 0 ? -1 : C.head->err_off;
    g->stream_err_off = -1;
    return;
  }
  // a unit of member m failed (m exists: a unit lies behind a header)
  const uint64_t raw = C.member_off[P.member_unit[m]] >> 3;
  g->n_members = m;
  g->err_off = (int64_t)P.member_off[m];
  g->stream_err_off = (rc == FLATE_HIP_E_CORRUPT && C.head->err_off >= 0) ? C.head->err_off - (int64_t)raw : -1;
}

// One thread per member, behind the checksums.  Judged only when every unit decoded.
__global__ __launch_bounds__(256) void gzfile_trailer_kernel(GzFileDecParams G) {
  const uint32_t m = blockIdx.x * 256u + threadIdx.x;
  if (m >= G.n_members) return;
  if (G.D.dh->first_bad != 0xffffffffu || G.D.dh->decode_bad != 0xffffffffu) return;
  const uint8_t *t = G.D.in + G.P.member_off[m + 1u] - kGzipTrailerLen;
  const uint32_t want = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
  const uint32_t isize = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
  const uint64_t size = G.P.member_out[m + 1u] - G.P.member_out[m];
  const uint32_t sum = size ? G.sums[m] : 0u;  // (the CRC-32 of nothing)
  if (sum != want || (uint32_t)size != isize) atomicMin(&G.v->bad_trailer, m);
}

// One thread: a disagreement of the two decodes, else the first failing unit's verdict, else the discovery's (a chain
// that broke at a header, a unit that is too large), else the first wrong trailer's.
__global__ void gzfile_verdict_kernel(GzFileDecParams G) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const OneDecParams &D = G.D;
  const GzFileHead g = *G.P.gh;
  GzFileVerdict *v = G.v;
  const uint32_t fb = D.dh->first_bad;
  v->out_len = D.total;
  v->status = 0;
  v->bad_member = 0xffffffffu;
  v->err_off = -1;
  v->stream_err_off = -1;
  v->n_members = g.n_members;
  v->n_units = G.n_good;
  if (D.dh->decode_bad != 0xffffffffu) {
    v->status = FLATE_HIP_E_INTERNAL;
    v->out_len = 0;
  } else if (fb != 0xffffffffu) {
    const uint32_t m = G.P.u_member[fb];
    const int32_t st = D.status[fb];
    v->status = st;
    v->bad_member = m;
    v->n_members = m;
    v->n_units = fb;
    v->err_off = (int64_t)G.P.member_off[m];
    if (st == FLATE_HIP_E_CORRUPT && D.err_off[fb] >= 0)
      v->stream_err_off = D.err_off[fb] - (int64_t)(D.unit_bit[G.P.member_unit[m]] >> 3);
    v->out_len = D.out_off[fb] + D.produced[fb];
  } else if (D.head->h.rc != 0) {
    v->status = D.head->h.rc;
    v->bad_member = g.n_members;
    v->err_off = g.err_off;
    v->stream_err_off = g.stream_err_off;
  } else if (v->bad_trailer != 0xffffffffu) {
    const uint32_t m = v->bad_trailer;
    v->status = FLATE_HIP_E_CORRUPT;
    v->bad_member = m;
    v->err_off = (int64_t)G.P.member_off[m];
    v->stream_err_off = (int64_t)(G.P.member_off[m + 1u] - G.P.member_off[m]);
  }
}

}  // namespace flate
