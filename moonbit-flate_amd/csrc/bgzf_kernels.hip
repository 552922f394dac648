// bgzf_kernels.hip -- member discovery for BGZF files (flate_hip_bgzf_index / flate_hip_bgzf_read): where the members
// of in[0, in_len) start and where their output goes, from the file's bytes alone (flate_kernels.h: BgzfParams).
//
// The result equals the serial walk from offset 0 (bgzf_rule.h: bgzf_serial_walk) on every input, also where
// compressed bytes look like member headers: such a decoy is a candidate like any other, it gets a successor like any
// other, and it is simply not on the path from candidate 0 -- unless the true chain leads to it, and then the serial
// walk goes there too.
//   bgzf_count_kernel   one workgroup per 4 KiB tile: 16-byte loads into LDS (the tiles lie on the 16-byte grid of the
//                       buffer's address; chunks that cross either end of the file are read byte by byte, nothing
//                       outside in[0, in_len) is touched), plus one chunk of halo for a header's first bytes; every
//                       thread tests its 16 offsets for the 4-byte magic in LDS and runs the member rule on the rare
//                       hit; the tile's count goes to tile_cnt
//   bgzf_scan_kernel    exclusive scan of the counts (one workgroup: scan_range of block_scan.h); n_cand
//   bgzf_fill_kernel    the same pass again, the hits written in file order (their places inside the tile:
//                       block_scan_excl of block_scan.h, which also adds up bgzf_count_kernel's count): cand_off,
//                       cand_total
//   bgzf_link_kernel    jump[0][c] = the candidate at cand_off[c] + cand_total[c] (binary search), the terminal node
//                       n_cand when that is in_len, else the dead node n_cand + 1; both absorb
//   bgzf_round_kernel   round j of pointer doubling: path[2^j + r] = jump[path[r]] for r < 2^j, jump = jump o jump
//   bgzf_finish_kernel  path rank r -> member_off[r], ISIZE; the thread whose successor is a sink writes the verdict
//   bgzf_out_scan_kernel  exclusive scan of ISIZE -> out_off (one workgroup, scan_range again)
// A successor lies strictly above its member, so nothing cycles; the host launches ceil(log2(cap + 2)) rounds.
#include <hip/hip_runtime.h>

#include "bgzf_rule.h"
#include "block_scan.h"
#include "flate_hip.h"
#include "flate_kernels.h"

namespace flate {

namespace {

constexpr uint32_t kChunks = kBgzfTile / 16;  // 256: one per thread

// the tile's bytes (kBgzfTile + 16 of halo) into LDS; bytes outside the file read as zero
__device__ inline void load_tile(const BgzfParams &P, uint8_t *lds, uint64_t v0, uint32_t A) {
  const uint64_t v_end = (uint64_t)A + P.in_len;  // virtual position = file offset + A: multiples of 16 are aligned
  for (uint32_t ch = threadIdx.x; ch <= kChunks; ch += 256u) {
    const uint64_t v = v0 + 16ull * ch;
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (v >= A && v + 16u <= v_end) {
      w = *reinterpret_cast<const uint4 *>(P.in + (v - A));
    } else if (v + 16u > A && v < v_end) {
      uint32_t d[4] = {0u, 0u, 0u, 0u};
      for (uint32_t b = 0; b < 16u; ++b) {
        const uint64_t vv = v + b;
        if (vv >= A && vv < v_end) d[b >> 2] |= (uint32_t)P.in[vv - A] << (8u * (b & 3u));
      }
      w = make_uint4(d[0], d[1], d[2], d[3]);
    }
    *reinterpret_cast<uint4 *>(lds + 16u * ch) = w;
  }
  __syncthreads();
}

// this thread's 16 offsets: bit b of the result = a member can be read at virtual position v0 + 16 * tid + b;
// totals[k]: the size of the k-th of them
__device__ inline uint32_t test_offsets(const BgzfParams &P, const uint8_t *lds, uint64_t v0, uint32_t A, uint32_t *totals) {
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

__device__ inline uint32_t buf_align(const BgzfParams &P) { return (uint32_t)(reinterpret_cast<uintptr_t>(P.in) & 15u); }

}  // namespace

__global__ __launch_bounds__(256) void bgzf_count_kernel(BgzfParams P) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kBgzfTile + 16];
  __shared__ uint32_t wtot[4];
  const uint32_t A = buf_align(P);
  const uint64_t v0 = (uint64_t)blockIdx.x * kBgzfTile;
  load_tile(P, lds, v0, A);
  uint32_t totals[6];  // (two hits are at least 3 bytes apart: at most 6 in 16 offsets)
  const uint32_t hits = test_offsets(P, lds, v0, A, totals);
  uint32_t sum = 0;
  (void)block_scan_excl<4, uint32_t>((uint32_t)__popc(hits), wtot, &sum);
  if (threadIdx.x == 0) P.tile_cnt[blockIdx.x] = sum;
}

// One workgroup: tile_cnt becomes its exclusive scan (n_tiles + 1 entries); the head is initialised.
__global__ __launch_bounds__(1024) void bgzf_scan_kernel(BgzfParams P) {
  __shared__ uint64_t wtot[16];
  // (above cap nothing downstream runs: the saturated value only has to stay above it)
  auto sat = [](uint64_t x) { return x > 0xffffffffull ? 0xffffffffu : (uint32_t)x; };
  const uint64_t n = scan_range<16, uint64_t>(
      P.n_tiles, wtot, [&](uint32_t i) { return (uint64_t)P.tile_cnt[i]; },
      [&](uint32_t i, uint64_t at, uint64_t) { P.tile_cnt[i] = sat(at); });
  if (threadIdx.x == 0) {
    P.tile_cnt[P.n_tiles] = sat(n);
    BgzfHead h;
    h.out_bytes = 0;
    h.err_off = 0;
    h.n_members = 0;
    h.rc = FLATE_HIP_E_CORRUPT;  // (until bgzf_finish_kernel has found the chain's end)
    h.eof_marker = 0;
    h.n_cand = sat(n);
    *P.head = h;
  }
}

__global__ __launch_bounds__(256) void bgzf_fill_kernel(BgzfParams P) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kBgzfTile + 16];
  __shared__ uint32_t wtot[4];
  if (P.head->n_cand > P.cap) return;  // (uniform: the arrays are too small, the host runs the pass again)
  const uint32_t first = P.tile_cnt[blockIdx.x];
  if (P.tile_cnt[blockIdx.x + 1] == first) return;  // (uniform: nothing in this tile)
  const uint32_t A = buf_align(P);
  const uint64_t v0 = (uint64_t)blockIdx.x * kBgzfTile;
  load_tile(P, lds, v0, A);
  uint32_t totals[6];
  const uint32_t hits = test_offsets(P, lds, v0, A, totals);
  uint32_t sum = 0;
  uint32_t at = first + block_scan_excl<4, uint32_t>((uint32_t)__popc(hits), wtot, &sum);
  uint32_t k = 0;
  for (uint32_t b = 0; b < 16u; ++b) {
    if (!((hits >> b) & 1u)) continue;
    if (at < P.cap) {
      P.cand_off[at] = v0 + 16u * threadIdx.x + b - A;
      P.cand_total[at] = totals[k];
    }
    ++at, ++k;
  }
}

// One thread per node (n_cand + 2 of them).
__global__ __launch_bounds__(256) void bgzf_link_kernel(BgzfParams P) {
  const uint32_t n = P.head->n_cand;
  if (n > P.cap) return;
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  const uint32_t term = n, dead = n + 1u;
  if (c == 0) P.path[0] = (n && P.cand_off[0] == 0ull) ? 0u : dead;  // the first member is at 0
  if (c > dead) return;
  uint32_t next = c;  // the two sinks absorb
  if (c < n) {
    const uint64_t want = P.cand_off[c] + P.cand_total[c];  // (<= in_len: the member rule)
    next = dead;
    if (want == P.in_len) {
      next = term;
    } else {
      uint32_t lo = c + 1u, hi = n;  // a successor lies strictly above its member
      for (int it = 0; it < 32 && lo < hi; ++it) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (P.cand_off[mid] < want) lo = mid + 1u;
        else hi = mid;
      }
      if (lo < n && P.cand_off[lo] == want) next = lo;
    }
  }
  P.jump[0][c] = next;
}

// Round j: the known path [0, 2^j) yields [2^j, 2^(j+1)) through jump[j & 1] (2^j steps), which is then squared into
// the other array.
__global__ __launch_bounds__(256) void bgzf_round_kernel(BgzfParams P, uint32_t j) {
  const uint32_t n = P.head->n_cand;
  if (n > P.cap) return;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t *cur = P.jump[j & 1u];
  uint32_t *nxt = P.jump[(j & 1u) ^ 1u];
  const uint32_t half = 1u << j;
  if (i < half && half + i < P.path_len) P.path[half + i] = cur[P.path[i]];
  if (i <= n + 1u) nxt[i] = cur[cur[i]];
}

__global__ __launch_bounds__(256) void bgzf_finish_kernel(BgzfParams P) {
  const uint32_t n = P.head->n_cand;
  if (n > P.cap) return;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r + 1u >= P.path_len) return;  // (the last entry is a sink: see below)
  const uint32_t c = P.path[r];
  if (c >= n) {
    // (rc stays FLATE_HIP_E_CORRUPT, err_off 0, n_members 0 when not even offset 0 holds a member)
    return;
  }
  const uint64_t off = P.cand_off[c];
  const uint32_t total = P.cand_total[c];
  const uint8_t *t = P.in + off + total - 4u;
  P.member_off[r] = off;
  P.isize[r] = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
  // (the chain holds at most n candidates and path_len >= n + 2: r + 1 is inside the path)
  const uint32_t succ = P.path[r + 1u];
  if (succ < n) return;
  BgzfHead *h = P.head;  // this is the last well-formed member: one thread gets here
  h->n_members = r + 1u;
  if (succ == n) {
    h->rc = 0;
    h->err_off = -1;
    h->eof_marker = bgzf_is_eof_marker(P.in + off, total) ? 1u : 0u;
    P.member_off[r + 1u] = P.in_len;
  } else {
    h->rc = FLATE_HIP_E_CORRUPT;
    h->err_off = (int64_t)(off + total);
  }
}

// One workgroup, behind bgzf_finish_kernel: out_off = the exclusive scan of the members' ISIZE.
__global__ __launch_bounds__(1024) void bgzf_out_scan_kernel(BgzfParams P) {
  __shared__ uint64_t wtot[16];
  if (P.head->n_cand > P.cap || P.head->rc != 0) return;  // (uniform)
  const uint32_t hi = P.head->n_members;
  const uint64_t total = scan_range<16, uint64_t>(
      hi, wtot, [&](uint32_t i) { return (uint64_t)P.isize[i]; },
      [&](uint32_t i, uint64_t before, uint64_t) { P.out_off[i] = before; });
  if (threadIdx.x == 0) {
    P.out_off[hi] = total;
    P.head->out_bytes = total;
  }
}

}  // namespace flate
