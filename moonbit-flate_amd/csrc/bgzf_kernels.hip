// bgzf_kernels.hip -- member discovery for BGZF files (flate_hip_bgzf_index / flate_hip_bgzf_read): where the members
// of in[0, in_len) start and where their output goes, from the file's bytes alone (flate_kernels.h: BgzfParams).
//
// The result equals the serial walk from offset 0 (bgzf_rule.h: bgzf_serial_walk) on every input, also where
// compressed bytes look like member headers: such a decoy is a candidate like any other, it gets a successor like any
// other, and it is simply not on the path from candidate 0 -- unless the true chain leads to it, and then the serial
// walk goes there too.
// The skeleton is chain_walk.h's (flate_kernels.h: THE DISCOVERY SKELETON); what is BGZF's own:
//   bgzf_count_kernel / bgzf_fill_kernel   the offset test: the 4-byte magic in LDS, the member rule (bgzf_rule.h) on
//                       the rare hit; a hit stores cand_off and cand_total
//   bgzf_link_kernel    a candidate ends at cand_off + cand_total; the last one ends at in_len
//   bgzf_finish_kernel  path rank r -> member_off[r], ISIZE; the thread whose successor is a sink writes the verdict
//   bgzf_out_scan_kernel  exclusive scan of ISIZE -> out_off (one workgroup, scan_range of block_scan.h)
#include <hip/hip_runtime.h>

#include "bgzf_rule.h"
#include "chain_walk.h"
#include "flate_hip.h"

namespace flate {

namespace {

// this thread's 16 offsets: bit b of the result = a member can be read at virtual position v0 + 16 * tid + b;
// totals[k]: the size of the k-th of them (two hits are at least 3 bytes apart: at most 6 in 16 offsets)
__device__ inline uint32_t test_offsets(const ChainParams &P, const uint8_t *lds, uint64_t v0, uint32_t A, uint32_t *totals) {
  uint32_t hits = 0, k = 0;
  const uint32_t at = 16u * threadIdx.x;
  for (uint32_t b = 0; b < 16u; ++b) {
    const uint8_t *l = lds + at + b;
    if (!bgzf_magic_ok(l[0], l[1], l[2], l[3])) continue;
    const uint64_t v = v0 + at + b;
    if (v < A) continue;  // (zero fill in front of the file cannot pass the magic; kept for the subtraction below)
    const uint64_t p = v - A;
    if (p >= P.in_len) continue;
    const uint32_t t = bgzf_member_total(P.in + p, P.in_len - p);
    if (t) hits |= 1u << b, totals[k++] = t;
  }
  return hits;
}

}  // namespace

__global__ __launch_bounds__(256) void bgzf_count_kernel(BgzfParams P) {
  __shared__ TileLds L;
  const uint32_t A = tile_align(P.C.in);
  const uint64_t v0 = (uint64_t)blockIdx.x * kTileBytes;
  uint32_t totals[6];
  tile_count(P.C, L, v0, [&](const uint8_t *lds) { return (uint32_t)__popc(test_offsets(P.C, lds, v0, A, totals)); });
}

__global__ __launch_bounds__(256) void bgzf_fill_kernel(BgzfParams P) {
  __shared__ TileLds L;
  const uint32_t A = tile_align(P.C.in);
  const uint64_t v0 = (uint64_t)blockIdx.x * kTileBytes;
  uint32_t first, totals[6];
  if (!tile_fill_load(P.C, L, v0, false, &first)) return;
  const uint32_t hits = test_offsets(P.C, L.bytes, v0, A, totals);
  tile_put16(hits, tile_fill_at(L, first, (uint32_t)__popc(hits)), P.C.cap, [&](uint32_t i, uint32_t b, uint32_t k) {
    P.C.cand_off[i] = v0 + 16u * threadIdx.x + b - A;
    P.cand_total[i] = totals[k];
  });
}

// One thread per node (n_cand + 2 of them).
__global__ __launch_bounds__(256) void bgzf_link_kernel(BgzfParams P) {
  const uint32_t n = P.C.head->n_cand;
  if (n > P.C.cap) return;
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  const uint64_t want = c < n ? P.C.cand_off[c] + P.cand_total[c] : 0ull;  // (<= in_len: the member rule)
  chain_link(P.C, n, c, true, want == P.C.in_len, want);
}

__global__ __launch_bounds__(256) void bgzf_finish_kernel(BgzfParams P) {
  const uint32_t n = P.C.head->n_cand;
  if (n > P.C.cap) return;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r + 1u >= P.C.path_len) return;  // (the last entry is a sink: see below)
  const uint32_t c = P.C.path[r];
  if (c >= n) {
    // (rc stays FLATE_HIP_E_CORRUPT, err_off 0, n_members 0 when not even offset 0 holds a member)
    return;
  }
  const uint64_t off = P.C.cand_off[c];
  const uint32_t total = P.cand_total[c];
  const uint8_t *t = P.C.in + off + total - 4u;
  P.C.member_off[r] = off;
  P.isize[r] = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
  // (the chain holds at most n candidates and path_len >= n + 2: r + 1 is inside the path)
  const uint32_t succ = P.C.path[r + 1u];
  if (succ < n) return;
  BgzfHead *h = P.C.head;  // this is the last well-formed member: one thread gets here
  h->n_members = r + 1u;
  if (succ == n) {
    h->rc = 0;
    h->err_off = -1;
    h->eof_marker = bgzf_is_eof_marker(P.C.in + off, total) ? 1u : 0u;
    P.C.member_off[r + 1u] = P.C.in_len;
  } else {
    h->rc = FLATE_HIP_E_CORRUPT;
    h->err_off = (int64_t)(off + total);
  }
}

// One workgroup, behind bgzf_finish_kernel: out_off = the exclusive scan of the members' ISIZE.
__global__ __launch_bounds__(1024) void bgzf_out_scan_kernel(BgzfParams P) {
  __shared__ uint64_t wtot[16];
  if (P.C.head->n_cand > P.C.cap || P.C.head->rc != 0) return;  // (uniform)
  const uint32_t hi = P.C.head->n_members;
  const uint64_t total = scan_range<16, uint64_t>(
      hi, wtot, [&](uint32_t i) { return (uint64_t)P.isize[i]; },
      [&](uint32_t i, uint64_t before, uint64_t) { P.C.out_off[i] = before; });
  if (threadIdx.x == 0) {
    P.C.out_off[hi] = total;
    P.C.head->out_bytes = total;
  }
}

}  // namespace flate
