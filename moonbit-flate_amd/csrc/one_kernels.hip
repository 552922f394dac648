// one_kernels.hip -- block discovery for ONE long DEFLATE stream (flate_hip_inflate_one_index): where the units of the
// raw stream inside in[0, in_len) start -- bit 0 and every dynamic block header the serial decode reaches -- and where
// their output goes, from the stream's bits alone (flate_kernels.h: OneParams; the rule: deflate_block_rule.h).
//
// The skeleton is chain_walk.h's (flate_kernels.h: THE DISCOVERY SKELETON), at bit granularity and, as for gzip
// members, with the candidate count read back behind the scan.  What is this format's own:
//   one_init_kernel      the one range {0, in_len}, and the raw stream of FLATE_HIP_WRAP_RAW: all of it
//   frame_parse_kernel   (frame_kernels.hip; zlib and gzip) the header's verdict and the raw stream's range
//   one_count_kernel / one_fill_kernel   the offset test: every thread tests its 128 BIT offsets -- 13 bits of a 32-bit
//                        window first, then the three counts and the code-length code, all in LDS (at most 81 bits from
//                        the byte: inside the halo) -- and runs the whole rule FROM GLOBAL MEMORY on the rare hit; bit 0
//                        of the raw stream is a candidate whatever it holds; a hit stores its bit, cand_off.  The loop
//                        over the 128 bits stays here: the byte formats' 16-bit mask does not hold them.  Templates on the
//                        unit rule (one_find_kernel.inc): <false> as above, instantiated here; <true> (option
//                        "one_stored_units"; one_stored_kernels.hip) with the stored-header rule at every bit as well,
//                        from the 6 bytes in LDS behind it
//   one_probe_kernel     (one_probe_kernel.inc) every candidate decoded to the next dynamic header: OneProbe
//   one_link_kernel      a candidate whose probe succeeded ends at end_bit; the last one ends with a final block
//   one_finish_kernel    path rank r -> unit_bit[r], the unit's size; the thread at which the path meets a sink writes
//                        the verdict, or asks for the tail probe
//   one_out_scan_kernel  the exclusive scan of the sizes -> out_off (one workgroup, scan_range of block_scan.h)
// A unit ends strictly above its start (a block header has three bits), so nothing cycles.  No kernel waits for
// another workgroup; every loop is bounded by the tile, by the candidate count or by 32 search steps.
#include <hip/hip_runtime.h>

#include "chain_walk.h"
#include "deflate_block_rule.h"
#include "flate_hip.h"
#include "window_compose.h"

namespace flate {

// {0, in_len} and the raw stream of a bare DEFLATE stream; frame_parse_kernel overwrites the latter for a container
__global__ void one_init_kernel(FrameOne *one, uint64_t in_len) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  FrameOne o{};
  o.in_off[1] = in_len;
  o.pay_off[1] = in_len;
  o.pay_end = in_len;
  o.dict_used = FLATE_HIP_NO_DICT;
  *one = o;
}

#include "one_find_kernel.inc"

// the default unit rule: dynamic headers alone (dynamic and stored headers: one_stored_kernels.hip)
template __global__ void one_count_kernel<false>(OneParams P);
template __global__ void one_fill_kernel<false>(OneParams P);

// One thread per node (n_cand + 2 of them).
__global__ __launch_bounds__(256) void one_link_kernel(OneParams P) {
  const uint32_t n = P.C.cap;
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c == 0) P.C.member_off[0] = 0ull;
  OneProbe pr{};
  if (c < n) pr = P.probe[c];
  chain_link(P.C, n, c, c < n && pr.status == 0, pr.final_block != 0u, pr.end_bit);
}

__global__ __launch_bounds__(256) void one_finish_kernel(OneParams P) {
  const uint32_t n = P.C.cap;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r + 1u >= P.C.path_len) return;  // (the last entry is a sink: see below)
  const uint32_t c = P.C.path[r];
  if (c >= n) return;
  BgzfHead *h = P.C.head;
  const OneProbe pr = P.probe[c];
  P.C.member_off[r] = P.C.cand_off[c];
  if (pr.status != 0) {  // the decode ends IN this unit: one thread gets here, or one gets below
    P.head->fail_out = pr.out;
    P.head->fail_unit = 1u;
    h->n_members = r;
    h->rc = pr.status;
    h->err_off = pr.err_off;
    return;
  }
  P.usize[r] = pr.out;
  // (the chain holds at most n candidates and path_len >= n + 2: r + 1 is inside the path)
  const uint32_t succ = P.C.path[r + 1u];
  if (succ < n) return;
  h->n_members = r + 1u;  // this is the last good unit
  P.C.member_off[r + 1u] = pr.end_bit;
  if (succ == n) {
    h->rc = 0;
    h->err_off = -1;
  } else {  // a header of a unit-starting type that is no candidate: the tail probe reads it as the serial decoder
    P.head->tail_bit = pr.end_bit;
    P.head->tail = 1u;
  }
}

// One workgroup, behind one_finish_kernel: out_off = the exclusive scan of what the units inflate to -- of a broken
// chain too (its good prefix).
__global__ __launch_bounds__(1024) void one_out_scan_kernel(OneParams P) {
  __shared__ uint64_t wtot[16];
  const uint32_t hi = P.C.head->n_members;
  const uint64_t total = scan_range<16, uint64_t>(
      hi, wtot, [&](uint32_t i) { return P.usize[i]; },
      [&](uint32_t i, uint64_t before, uint64_t) { P.C.out_off[i] = before; });
  if (threadIdx.x == 0) {
    P.C.out_off[hi] = total;
    P.head->prefix_bytes = total;
    P.C.head->out_bytes = P.C.head->rc == 0 ? total : 0ull;
  }
}

// ---- the decode's scan (flate_hip_inflate_one; OneDecParams) ----

// One step of the scan over the round's tail functions: dst[k] = src[k] o src[k - s] for k >= s.  One thread per entry.
__global__ __launch_bounds__(256) void one_compose_kernel(const uint16_t *src, uint16_t *dst, uint32_t count, uint32_t s) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t k = idx / kWinEntries;
  if (k >= count) return;
  const uint16_t e = src[idx];
  dst[idx] = k >= s ? wc_compose(e, src + (k - s) * kWinEntries) : e;
}

// R[k + 1] = F[k] applied to the seed R[0], where F[k] is the composition of the round's functions up to unit k.
__global__ __launch_bounds__(256) void one_resolve_kernel(const uint16_t *F, uint8_t *R, uint32_t count) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (idx / kWinEntries >= count) return;
  R[kWinEntries + idx] = wc_resolve(F[idx], R);
}

// One thread per unit of the round (and one more): the round as spliced pieces with dictionaries.  Piece i's slot is
// the unit's range of the output; the first failing unit's slot ends at its failure (the bytes in front are delivered)
// and the units behind it get an empty slot: the decoder stops at their first token and writes nothing.  No slot
// reaches beyond `total`.
__global__ __launch_bounds__(256) void one_pieces_kernel(OneDecParams D) {
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
  const uint64_t have = at + D.hist_base;  // (hist_base <= kWinEntries: a part's history in front of out_off[0])
  const uint32_t dict_len = have < (uint64_t)kWinEntries ? (uint32_t)have : kWinEntries;
  D.p_dict_len[i] = dict_len;
  D.p_dict_at[i] = (uint64_t)(i + 1u) * kWinEntries - dict_len;  // the tail of R[i]; R[i + 1] follows it
}

// One thread per unit of the round, behind DECODE: a unit in front of the first failing one decodes without error to
// exactly its slot, or TAIL, the scan and DECODE disagree (the verdict is FLATE_HIP_E_INTERNAL then).  The failing
// unit's verdict is TAIL's.
__global__ __launch_bounds__(256) void one_check_kernel(OneDecParams D) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= D.count) return;
  const uint32_t u = D.u0 + i;
  if (u >= D.dh->first_bad) return;
  if (D.d_status[i] != 0 || D.d_out_len[i] != D.p_out_off[i + 1u] - D.p_out_off[i]) atomicMin(&D.dh->decode_bad, u);
}

// One thread: a disagreement of the two decodes, else the first failing unit's verdict, else the header's (a chain that stopped at a refused header), else the
// trailer's.
__global__ void one_verdict_kernel(OneDecParams D) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  OneDecHead *dh = D.dh;
  const uint32_t fb = dh->first_bad;
  dh->out_len = D.total;
  dh->status = 0;
  dh->err_off = -1;
  if (dh->decode_bad != 0xffffffffu) {
    dh->status = FLATE_HIP_E_INTERNAL;
    dh->out_len = 0;
  } else if (fb != 0xffffffffu) {
    dh->status = D.status[fb];
    dh->err_off = D.err_off[fb];
    dh->out_len = D.out_off[fb] + D.produced[fb];
  } else if (D.head->h.rc != 0) {
    dh->status = D.head->h.rc;
    dh->err_off = D.head->h.err_off;
  } else if (D.wrap != FLATE_HIP_WRAP_RAW) {
    const uint32_t empty = D.wrap == FLATE_HIP_WRAP_ZLIB ? 1u : 0u;  // the sums of nothing
    const uint32_t sum = D.sum ? *D.sum : empty;
    const uint32_t isize_off = D.wrap == FLATE_HIP_WRAP_GZIP ? ((uint32_t)D.total ^ D.one->isize) : 0u;
    if (((sum ^ D.one->want) | isize_off) != 0u) {
      dh->status = FLATE_HIP_E_CORRUPT;
      dh->err_off = (int64_t)D.in_len;
    }
  }
}

}  // namespace flate
