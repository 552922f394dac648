// gzip_kernels.hip -- member discovery for plain multi-member gzip files (flate_hip_gzip_index / flate_hip_gzip_read):
// where the members of in[0, in_len) start and where their output goes, from the file's bytes alone, although no
// member says how long it is (flate_kernels.h: GzipParams; the rule and the walk that defines every result: gzip_rule.h).
//
// The shape is bgzf_kernels.hip's, with one step more: a candidate's length comes from a size-only decode of every
// candidate at once, between the fill and the link.
//   gzip_count_kernel    one workgroup per 4 KiB tile, as bgzf_count_kernel: 16-byte loads into LDS on the grid of the
//                        buffer's address (chunks that cross either end of the file byte by byte, nothing outside
//                        in[0, in_len) is touched) plus one chunk of halo; every thread tests its 16 offsets for the
//                        3-byte magic and the reserved FLG bits in LDS and runs the header rule FROM GLOBAL MEMORY on the
//                        rare hit (a header can be longer than any halo); the tile's count goes to tile_cnt
//   bgzf_scan_kernel     (bgzf_kernels.hip) the exclusive scan of the counts; n_cand, which the host reads back: the
//                        launches that follow have one thread, or one wavefront, per candidate
//   gzip_fill_kernel     the same pass again, the hits written in file order: cand_off, cand_end
//   frame_parse_kernel   (frame_kernels.hip) over the candidates' ranges: pay_off, pay_end
//   the batch decoders   ONE size-only launch over all candidates (InfParams::used): status, out_len, used.  Nothing is
//                        stored, so a decoy can write nothing
//   gzip_link_kernel     jump[0][c] = the candidate at pay_off[c] + used[c] + 8 (binary search), the terminal node n_cand
//                        when that is in_len, else -- or when the decode failed -- the dead node n_cand + 1; both absorb
//   bgzf_round_kernel    (bgzf_kernels.hip) pointer doubling
//   gzip_finish_kernel   path rank r -> member_off[r], the member's size; the thread at which the path meets a sink
//                        writes the verdict
//   gzip_out_scan_kernel the exclusive scan of the sizes -> out_off (one workgroup, scan_range)
// A successor lies strictly above its member, so nothing cycles.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "flate_hip.h"
#include "flate_kernels.h"
#include "gzip_rule.h"

namespace flate {

namespace {

constexpr uint32_t kChunks = kBgzfTile / 16;  // 256: one per thread

__device__ inline uint32_t buf_align(const GzipParams &P) { return (uint32_t)(reinterpret_cast<uintptr_t>(P.B.in) & 15u); }

// the tile's bytes (kBgzfTile + 16 of halo) into LDS; bytes outside the file read as zero.  (bgzf_kernels.hip's
// load_tile: virtual position = file offset + A, so that multiples of 16 are aligned addresses.)
__device__ inline void load_tile(const GzipParams &P, uint8_t *lds, uint64_t v0, uint32_t A) {
  const uint8_t *in = P.B.in;
  const uint64_t v_end = (uint64_t)A + P.B.in_len;
  for (uint32_t ch = threadIdx.x; ch <= kChunks; ch += 256u) {
    const uint64_t v = v0 + 16ull * ch;
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (v >= A && v + 16u <= v_end) {
      w = *reinterpret_cast<const uint4 *>(in + (v - A));
    } else if (v + 16u > A && v < v_end) {
      uint32_t d[4] = {0u, 0u, 0u, 0u};
      for (uint32_t b = 0; b < 16u; ++b) {
        const uint64_t vv = v + b;
        if (vv >= A && vv < v_end) d[b >> 2] |= (uint32_t)in[vv - A] << (8u * (b & 3u));
      }
      w = make_uint4(d[0], d[1], d[2], d[3]);
    }
    *reinterpret_cast<uint4 *>(lds + 16u * ch) = w;
  }
  __syncthreads();
}

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
    if (p >= P.B.in_len) continue;
    if (gzip_header_len(P.B.in + p, gzip_range_end(p, P.B.in_len, P.member_max) - p)) hits |= 1u << b;
  }
  return hits;
}

// did candidate c's size-only decode reach the end of a final block?
__device__ inline bool cand_alive(const GzipParams &P, uint32_t c) { return P.bad[c] == 0u && P.status[c] == 0; }

}  // namespace

__global__ __launch_bounds__(256) void gzip_count_kernel(GzipParams P) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kBgzfTile + 16];
  __shared__ uint32_t wtot[4];
  const uint32_t A = buf_align(P);
  const uint64_t v0 = (uint64_t)blockIdx.x * kBgzfTile;
  load_tile(P, lds, v0, A);
  const uint32_t hits = test_offsets(P, lds, v0, A);
  uint32_t sum = 0;
  (void)block_scan_excl<4, uint32_t>((uint32_t)__popc(hits), wtot, &sum);
  if (threadIdx.x == 0) P.B.tile_cnt[blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void gzip_fill_kernel(GzipParams P) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kBgzfTile + 16];
  __shared__ uint32_t wtot[4];
  const uint32_t cap = P.B.cap;
  if (P.B.head->n_cand != cap) return;  // (uniform, never: the arrays are sized from the count the host read back)
  // (frame_parse_kernel reads one entry behind the last candidate)
  if (blockIdx.x == 0 && threadIdx.x == 0) P.B.cand_off[cap] = P.B.in_len;
  const uint32_t first = P.B.tile_cnt[blockIdx.x];
  if (P.B.tile_cnt[blockIdx.x + 1] == first) return;  // (uniform: nothing in this tile)
  const uint32_t A = buf_align(P);
  const uint64_t v0 = (uint64_t)blockIdx.x * kBgzfTile;
  load_tile(P, lds, v0, A);
  const uint32_t hits = test_offsets(P, lds, v0, A);
  uint32_t sum = 0;
  uint32_t at = first + block_scan_excl<4, uint32_t>((uint32_t)__popc(hits), wtot, &sum);
  for (uint32_t b = 0; b < 16u; ++b) {
    if (!((hits >> b) & 1u)) continue;
    if (at < cap) {
      const uint64_t p = v0 + 16u * threadIdx.x + b - A;
      P.B.cand_off[at] = p;
      P.cand_end[at] = gzip_range_end(p, P.B.in_len, P.member_max);
    }
    ++at;
  }
}

// One thread per node (n_cand + 2 of them).
__global__ __launch_bounds__(256) void gzip_link_kernel(GzipParams P) {
  const uint32_t n = P.B.cap;
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  const uint32_t term = n, dead = n + 1u;
  if (c == 0) {
    P.B.path[0] = (n && P.B.cand_off[0] == 0ull) ? 0u : dead;  // the first member is at 0
    P.B.member_off[0] = 0ull;
  }
  if (c > dead) return;
  uint32_t next = c;  // the two sinks absorb
  if (c < n) {
    next = dead;
    if (cand_alive(P, c)) {
      const uint64_t want = P.pay_off[c] + P.used[c] + kGzipTrailerLen;  // (<= cand_end[c]: the decoder's range)
      if (want == P.B.in_len) {
        next = term;
      } else {
        uint32_t lo = c + 1u, hi = n;  // a successor lies strictly above its member
        for (int it = 0; it < 32 && lo < hi; ++it) {
          const uint32_t mid = lo + (hi - lo) / 2u;
          if (P.B.cand_off[mid] < want) lo = mid + 1u;
          else hi = mid;
        }
        if (lo < n && P.B.cand_off[lo] == want) next = lo;
      }
    }
  }
  P.B.jump[0][c] = next;
}

__global__ __launch_bounds__(256) void gzip_finish_kernel(GzipParams P) {
  const uint32_t n = P.B.cap;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r + 1u >= P.B.path_len) return;  // (the last entry is a sink: see below)
  const uint32_t c = P.B.path[r];
  if (c >= n) {
    // (rc stays FLATE_HIP_E_CORRUPT, err_off 0, n_members 0 when not even offset 0 holds a header)
    return;
  }
  BgzfHead *h = P.B.head;
  const uint64_t off = P.B.cand_off[c];
  P.B.member_off[r] = off;
  if (!cand_alive(P, c)) {  // the walk ends AT this candidate: one thread gets here, or one gets below
    h->n_members = r;
    h->rc = P.bad[c] ? FLATE_HIP_E_CORRUPT : gzip_dead_code(P.status[c], off, P.B.in_len, P.member_max);
    h->err_off = (int64_t)off;
    return;
  }
  P.msize[r] = P.out_len[c];
  // (the chain holds at most n candidates and path_len >= n + 2: r + 1 is inside the path)
  const uint32_t succ = P.B.path[r + 1u];
  if (succ < n) return;
  const uint64_t end = P.pay_off[c] + P.used[c] + kGzipTrailerLen;
  h->n_members = r + 1u;  // this is the last good member
  P.B.member_off[r + 1u] = end;
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
  const uint32_t hi = P.B.head->n_members;
  const uint64_t total = scan_range<16, uint64_t>(
      hi, wtot, [&](uint32_t i) { return P.msize[i]; },
      [&](uint32_t i, uint64_t before, uint64_t) { P.B.out_off[i] = before; });
  if (threadIdx.x == 0) {
    P.B.out_off[hi] = total;
    P.B.head->out_bytes = P.B.head->rc == 0 ? total : 0ull;
  }
}

}  // namespace flate
