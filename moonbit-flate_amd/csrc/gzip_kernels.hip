// gzip_kernels.hip -- member discovery for plain multi-member gzip files (flate_hip_gzip_index / flate_hip_gzip_read):
// where the members of in[0, in_len) start and where their output goes, from the file's bytes alone, although no
// member says how long it is (flate_kernels.h: GzipParams; the rule and the walk that defines every result: gzip_rule.h).
//
// The skeleton is chain_walk.h's (flate_kernels.h: THE DISCOVERY SKELETON), with one step more: a candidate's length
// comes from a size-only decode of every candidate at once, between the fill and the link.  What is gzip's own:
//   gzip_count_kernel / gzip_fill_kernel   the offset test: the 3-byte magic and the reserved FLG bits in LDS, the
//                        header rule FROM GLOBAL MEMORY on the rare hit (a header can be longer than any halo); a hit
//                        stores cand_off and cand_end.  The host reads n_cand back behind the scan: the launches that
//                        follow have one thread, or one wavefront, per candidate
//   frame_parse_kernel   (frame_kernels.hip) over the candidates' ranges: pay_off, pay_end
//   the batch decoders   ONE size-only launch over all candidates (InfParams::used): status, out_len, used.  Nothing is
//                        stored, so a decoy can write nothing
//   gzip_link_kernel     a candidate whose decode ended a final block ends at pay_off + used + 8; the last one ends at
//                        in_len
//   gzip_finish_kernel   path rank r -> member_off[r], the member's size; the thread at which the path meets a sink
//                        writes the verdict
//   gzip_out_scan_kernel the exclusive scan of the sizes -> out_off (one workgroup, scan_range of block_scan.h)
#include <hip/hip_runtime.h>

#include "chain_walk.h"
#include "flate_hip.h"
#include "gzip_rule.h"

namespace flate {

namespace {

// this thread's 16 offsets: bit b of the result = a member can start at virtual position v0 + 16 * tid + b
__device__ inline uint32_t test_offsets(const GzipParams &P, const uint8_t *lds, uint64_t v0, uint32_t A) {
  uint32_t hits = 0;
  const uint32_t at = 16u * threadIdx.x;
  for (uint32_t b = 0; b < 16u; ++b) {
    const uint8_t *l = lds + at + b;
    if (!gzip_magic_ok(l[0], l[1], l[2], l[3])) continue;
    const uint64_t v = v0 + at + b;
    if (v < A) continue;  // (zero fill in front of the file cannot pass the magic; kept for the subtraction below)
    const uint64_t p = v - A;
    if (p >= P.C.in_len) continue;
    if (gzip_header_len(P.C.in + p, gzip_range_end(p, P.C.in_len, P.member_max) - p)) hits |= 1u << b;
  }
  return hits;
}

// did candidate c's size-only decode reach the end of a final block?
__device__ inline bool cand_alive(const GzipParams &P, uint32_t c) { return P.bad[c] == 0u && P.status[c] == 0; }

}  // namespace

__global__ __launch_bounds__(256) void gzip_count_kernel(GzipParams P) {
  __shared__ TileLds L;
  const uint32_t A = tile_align(P.C.in);
  const uint64_t v0 = (uint64_t)blockIdx.x * kTileBytes;
  tile_count(P.C, L, v0, [&](const uint8_t *lds) { return (uint32_t)__popc(test_offsets(P, lds, v0, A)); });
}

__global__ __launch_bounds__(256) void gzip_fill_kernel(GzipParams P) {
  __shared__ TileLds L;
  const uint32_t A = tile_align(P.C.in), cap = P.C.cap;
  const uint64_t v0 = (uint64_t)blockIdx.x * kTileBytes;
  // (frame_parse_kernel reads one entry behind the last candidate)
  if (P.C.head->n_cand == cap && blockIdx.x == 0 && threadIdx.x == 0) P.C.cand_off[cap] = P.C.in_len;
  uint32_t first;
  if (!tile_fill_load(P.C, L, v0, true, &first)) return;
  const uint32_t hits = test_offsets(P, L.bytes, v0, A);
  tile_put16(hits, tile_fill_at(L, first, (uint32_t)__popc(hits)), cap, [&](uint32_t i, uint32_t b, uint32_t) {
    const uint64_t p = v0 + 16u * threadIdx.x + b - A;
    P.C.cand_off[i] = p;
    P.cand_end[i] = gzip_range_end(p, P.C.in_len, P.member_max);
  });
}

// One thread per node (n_cand + 2 of them).
__global__ __launch_bounds__(256) void gzip_link_kernel(GzipParams P) {
  const uint32_t n = P.C.cap;
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c == 0) P.C.member_off[0] = 0ull;
  const bool alive = c < n && cand_alive(P, c);
  const uint64_t want = alive ? P.pay_off[c] + P.used[c] + kGzipTrailerLen : 0ull;  // (<= cand_end[c]: the decoder's range)
  chain_link(P.C, n, c, alive, want == P.C.in_len, want);
}

__global__ __launch_bounds__(256) void gzip_finish_kernel(GzipParams P) {
  const uint32_t n = P.C.cap;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r + 1u >= P.C.path_len) return;  // (the last entry is a sink: see below)
  const uint32_t c = P.C.path[r];
  if (c >= n) {
    // (rc stays FLATE_HIP_E_CORRUPT, err_off 0, n_members 0 when not even offset 0 holds a header)
    return;
  }
  BgzfHead *h = P.C.head;
  const uint64_t off = P.C.cand_off[c];
  P.C.member_off[r] = off;
  if (!cand_alive(P, c)) {  // the walk ends AT this candidate: one thread gets here, or one gets below
    h->n_members = r;
    h->rc = P.bad[c] ? FLATE_HIP_E_CORRUPT : gzip_dead_code(P.status[c], off, P.C.in_len, P.member_max);
    h->err_off = (int64_t)off;
    return;
  }
  P.msize[r] = P.out_len[c];
  // (the chain holds at most n candidates and path_len >= n + 2: r + 1 is inside the path)
  const uint32_t succ = P.C.path[r + 1u];
  if (succ < n) return;
  const uint64_t end = P.pay_off[c] + P.used[c] + kGzipTrailerLen;
  h->n_members = r + 1u;  // this is the last good member
  P.C.member_off[r + 1u] = end;
  if (succ == n) {
    h->rc = 0;
    h->err_off = -1;
  } else {  // no member can start where this one ends
    h->rc = FLATE_HIP_E_CORRUPT;
    h->err_off = (int64_t)end;
  }
}

// One workgroup, behind gzip_finish_kernel: out_off = the exclusive scan of what the members inflate to -- of a broken
// chain too (its good prefix).
__global__ __launch_bounds__(1024) void gzip_out_scan_kernel(GzipParams P) {
  __shared__ uint64_t wtot[16];
  const uint32_t hi = P.C.head->n_members;
  const uint64_t total = scan_range<16, uint64_t>(
      hi, wtot, [&](uint32_t i) { return P.msize[i]; },
      [&](uint32_t i, uint64_t before, uint64_t) { P.C.out_off[i] = before; });
  if (threadIdx.x == 0) {
    P.C.out_off[hi] = total;
    P.C.head->out_bytes = P.C.head->rc == 0 ? total : 0ull;
  }
}

}  // namespace flate
