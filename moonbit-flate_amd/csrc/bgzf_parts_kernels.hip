// bgzf_parts_kernels.hip -- a PART of a BGZF file (flate_hip_bgzf_reader_read): the two kernels behind the discovery of
// bgzf_kernels.hip that are the part's own (flate_kernels.h: BgzfPartParams).  Count, scan, fill, link and the rounds of
// pointer doubling are the whole file's kernels, unchanged: a member the part cuts fails the member rule (its total runs
// past in_len), so it is no candidate, and the chain from candidate 0 ends in the dead node where the serial walk over
// the part finds no member.
//   bgzf_part_finish_kernel    path rank r -> member_off[r], ISIZE; the thread whose successor is a sink writes THE
//                              PART STOP (bgzf_parts_rule.h) where the whole file's kernel writes its verdict
//   bgzf_part_out_scan_kernel  exclusive scan of ISIZE -> out_off, DELIVERY (the clip to out_cap and index_cap), the
//                              result words, the FILE-absolute index (one workgroup, scan_range of block_scan.h)
#include <hip/hip_runtime.h>

#include "bgzf_parts_rule.h"
#include "bgzf_rule.h"
#include "chain_walk.h"
#include "flate_hip.h"

namespace flate {

__global__ __launch_bounds__(256) void bgzf_part_finish_kernel(BgzfPartParams Q) {
  const BgzfParams &P = Q.B;
  const uint32_t n = P.C.head->n_cand;
  if (n > P.C.cap) return;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r + 1u >= P.C.path_len) return;  // (the last entry is a sink)
  const uint32_t c = P.C.path[r];
  BgzfPartFound *f = Q.found;
  if (c >= n) {
    if (r == 0) {  // not even offset 0 holds a member: the stop at p = 0 (in_len > 0: never a boundary)
      f->n = 0;
      f->p = 0;
      f->stop = bgzf_part_stop(P.C.in_len, Q.final_in != 0);
      P.C.member_off[0] = 0;
    }
    return;
  }
  const uint64_t off = P.C.cand_off[c];
  const uint32_t total = P.cand_total[c];
  const uint8_t *t = P.C.in + off + total - 4u;
  P.C.member_off[r] = off;
  P.isize[r] = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
  // (the chain holds at most n candidates and path_len >= n + 2: r + 1 is inside the path)
  if (P.C.path[r + 1u] < n) return;
  // this is the last whole member of the part: one thread gets here.  Its successor is the terminal node (it ends at
  // in_len: avail == 0) or the dead node (no member at p)
  const uint64_t p = off + total;
  f->n = r + 1u;
  f->p = p;
  f->stop = bgzf_part_stop(P.C.in_len - p, Q.final_in != 0);
  P.C.member_off[r + 1u] = p;
}

// One workgroup, behind bgzf_part_finish_kernel.  The members' output offsets are the exclusive scan of ISIZE; member i
// is delivered where bgzf_part_delivers says so, which is a prefix of the members: k and the bytes it inflates to are
// the maxima over the delivered ones (LDS atomics: one per member).  The index in FILE coordinates is written for all n
// members; the host reads back the k + 1 entries of the delivered ones only.
__global__ __launch_bounds__(1024) void bgzf_part_out_scan_kernel(BgzfPartParams Q) {
  __shared__ uint64_t wtot[16];
  __shared__ unsigned long long end_s;
  __shared__ uint32_t k_s;
  const BgzfParams &P = Q.B;
  if (P.C.head->n_cand > P.C.cap) return;  // (uniform)
  const uint32_t n = Q.found->n;
  if (threadIdx.x == 0) k_s = 0, end_s = 0;
  __syncthreads();
  const uint64_t total = scan_range<16, uint64_t>(
      n, wtot, [&](uint32_t i) { return (uint64_t)P.isize[i]; },
      [&](uint32_t i, uint64_t before, uint64_t v) {
        P.C.out_off[i] = before;
        Q.idx_out_off[i] = Q.base_out + before;
        Q.idx_member_off[i] = Q.base_in + P.C.member_off[i];
        if (bgzf_part_delivers(i, before + v, Q.out_cap, Q.k_max)) {
          atomicMax(&k_s, i + 1u);
          atomicMax(&end_s, (unsigned long long)(before + v));
        }
      });
  __syncthreads();  // (k_s and end_s are final)
  if (threadIdx.x != 0) return;
  P.C.out_off[n] = total;
  Q.idx_out_off[n] = Q.base_out + total;
  Q.idx_member_off[n] = Q.base_in + P.C.member_off[n];
  const uint32_t k = k_s;
  BgzfPartFound *f = Q.found;
  f->k = k;
  f->in_end = P.C.member_off[k];
  f->out_end = end_s;
  f->isize0 = n ? (uint64_t)P.isize[0] : 0ull;
  uint32_t eof = 0;
  if (k) {
    const uint64_t a = P.C.member_off[k - 1u];
    eof = bgzf_is_eof_marker(P.C.in + a, (uint32_t)(P.C.member_off[k] - a)) ? 1u : 0u;
  }
  f->eof_last = eof;
}

}  // namespace flate
