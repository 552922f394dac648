// bgzf_range_kernels.hip -- random access into a BGZF file (flate_hip_bgzf_read_ranges): from a batch of ranges to the
// members they touch and to the places of the requested bytes, on the index the discovery kernels left on the device
// (flate_kernels.h: BgzfRangeParams), and the gather of the decoded bytes into the caller's buffer (BgzfGatherParams).
//   bgzf_range_locate_kernel  one thread per range: the range rule (bgzf_range_rule.h) -- byte positions clamped to
//                             the file's size, virtual offsets looked up in member_off by binary search and checked --
//                             gives b, the length, the status and the first and last member that hold bytes of it; a
//                             non-empty range adds +1 at its first member and -1 behind its last one to a difference
//                             array (vector atomics): no walk over the range's span, which may be the whole file
//   bgzf_range_select_kernel  one workgroup over the members: the scan of the differences says whether any range
//                             covers member k; masked with ISIZE > 0, one scan of (1, ISIZE) gives the selected
//                             members their rank and their place in the dense scratch; compacted in file order
//                             (three dependent block_scan_excl of block_scan.h per chunk, the carries in registers)
//   bgzf_range_layout_kernel  one workgroup over the ranges: the scan of their lengths (their places in `out`;
//                             scan_range of block_scan.h); every
//                             member with bytes inside a range is selected, so the range's bytes are ONE run of the
//                             scratch, starting at scratch_at[first] + (b - out_off[first])
//   bgzf_gather_kernel        the runs into `out`.  No LDS: 16-byte stores on the destination's 16-byte grid, the
//                             source bytes from two aligned 16-byte loads realigned in registers (v_alignbyte), heads
//                             and tails byte by byte.  Work is cut by cost = bytes + 256 per range into windows of
//                             64 KiB, one workgroup each, found by binary search in the ranges' places: a long run is
//                             cut on the destination's grid into pieces that all 256 threads copy, short runs go one
//                             per wavefront.  Nothing outside out[r_out_off[r], r_out_off[r + 1]) is written for r.
// No kernel waits for another workgroup; every loop is bounded by n_members, n_ranges or the window.
#include <hip/hip_runtime.h>

#include "bgzf_range_rule.h"
#include "block_scan.h"
#include "flate_hip.h"
#include "flate_kernels.h"

namespace flate {

__global__ __launch_bounds__(256) void bgzf_range_locate_kernel(BgzfRangeParams P) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= P.n_ranges) return;
  const BgzfRangeLoc L = bgzf_range_locate(P.pos_kind, P.begin[r], P.end[r], P.member_off, P.out_off_m, P.n_members);
  P.r_b[r] = L.b;
  P.r_len[r] = L.e - L.b;
  P.r_status[r] = L.status == 0 ? FLATE_HIP_OK : FLATE_HIP_E_INVALID;
  P.r_first[r] = L.first;
  P.r_last[r] = L.last;
  if (L.first != kBgzfNoMember) {  // (first <= last < n_members: the array has n_members + 1 entries)
    atomicAdd(&P.diff[L.first], 1);
    atomicAdd(&P.diff[L.last + 1u], -1);
  }
}

__global__ __launch_bounds__(1024) void bgzf_range_select_kernel(BgzfRangeParams P) {
  __shared__ int64_t wtot[16];
  int64_t cover_c = 0, cnt_c = 0, bytes_c = 0;  // the three sums over the chunks in front
  for (uint32_t base = 0; base < P.n_members; base += 1024u) {
    const uint32_t k = base + threadIdx.x;
    const bool in = k < P.n_members;
    const int64_t d = in ? (int64_t)P.diff[k] : 0;
    int64_t dsum, csum, bsum;
    const int64_t cover = cover_c + block_scan_excl<16, int64_t>(d, wtot, &dsum) + d;  // ranges that cover member k
    const uint32_t isize = in ? P.isize[k] : 0u;
    const bool sel = in && cover > 0 && isize > 0u;
    const uint64_t rank = (uint64_t)(cnt_c + block_scan_excl<16, int64_t>(sel ? 1 : 0, wtot, &csum));
    const uint64_t at = (uint64_t)(bytes_c + block_scan_excl<16, int64_t>(sel ? (int64_t)isize : 0, wtot, &bsum));
    if (in) {
      P.rank[k] = (uint32_t)rank;
      P.scratch_at[k] = at;
    }
    if (sel) {
      BgzfSel s;
      s.in_off = P.member_off[k];
      s.in_end = P.member_off[k + 1u];
      s.scratch_off = at;
      s.member = k;
      s.isize = isize;
      P.sel[rank] = s;
    }
    cover_c += dsum, cnt_c += csum, bytes_c += bsum;
  }
  if (threadIdx.x == 0) {
    P.head->n_sel = (uint32_t)cnt_c;
    P.head->scratch_total = (uint64_t)bytes_c;
  }
}

__global__ __launch_bounds__(1024) void bgzf_range_layout_kernel(BgzfRangeParams P) {
  __shared__ int64_t wtot[16];
  __shared__ uint32_t invalid_s;
  if (threadIdx.x == 0) invalid_s = 0u;
  __syncthreads();
  const uint64_t total = (uint64_t)scan_range<16, int64_t>(
      P.n_ranges, wtot, [&](uint32_t r) { return (int64_t)P.r_len[r]; },
      [&](uint32_t r, int64_t at, int64_t) {
        const uint32_t first = P.r_first[r], last = P.r_last[r];
        P.r_out_off[r] = (uint64_t)at;
        if (first != kBgzfNoMember) {
          P.r_src[r] = P.scratch_at[first] + (P.r_b[r] - P.out_off_m[first]);
          P.r_rank_lo[r] = P.rank[first];
          P.r_rank_hi[r] = P.rank[last] + 1u;
        } else {
          P.r_src[r] = 0ull;
          P.r_rank_lo[r] = 0u;
          P.r_rank_hi[r] = 0u;
        }
        if (P.r_status[r] != 0) atomicOr(&invalid_s, 1u);
      });
  __syncthreads();  // (the last chunk's flags)
  if (threadIdx.x == 0) {
    P.r_out_off[P.n_ranges] = total;
    P.head->out_total = total;
    P.head->any_invalid = invalid_s;
  }
}

// ---- the gather ----

namespace {

// dst[0, len) = src[0, len) by the lanes t = 0 .. lanes - 1 (a wavefront, or the whole workgroup).  dst and src at any
// alignment; the aligned 16-byte loads touch at most 15 bytes in front of src and 31 behind src + len, inside the
// scratch allocation (BgzfGatherParams).
template <uint32_t DW>
__device__ inline void copy_body(uint4 *d, const uint4 *sa, uint32_t b, uint32_t chunks, uint32_t t, uint32_t lanes) {
  for (uint32_t j = t; j < chunks; j += lanes) {
    const uint4 lo = sa[j], hi = sa[j + 1u];
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    d[j] = make_uint4(__builtin_amdgcn_alignbyte(w[DW + 1], w[DW], b), __builtin_amdgcn_alignbyte(w[DW + 2], w[DW + 1], b),
                      __builtin_amdgcn_alignbyte(w[DW + 3], w[DW + 2], b), __builtin_amdgcn_alignbyte(w[DW + 4], w[DW + 3], b));
  }
}

__device__ inline void copy_piece(uint8_t *dst, const uint8_t *src, uint32_t len, uint32_t t, uint32_t lanes) {
  if (len < 32u) {
    for (uint32_t i = t; i < len; i += lanes) dst[i] = src[i];
    return;
  }
  const uint32_t head = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
  const uint32_t chunks = (len - head) >> 4;
  const uint32_t tail_at = head + 16u * chunks;
  const uint32_t edge = head + (len - tail_at);  // the bytes off the destination's grid: at most 30
  for (uint32_t i = t; i < edge; i += lanes) {
    const uint32_t at = i < head ? i : tail_at + (i - head);
    dst[at] = src[at];
  }
  const uint8_t *s = src + head;
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 15u);
  uint4 *d = reinterpret_cast<uint4 *>(dst + head);
  const uint4 *sa = reinterpret_cast<const uint4 *>(s - sh);
  if (sh == 0u) {
    for (uint32_t j = t; j < chunks; j += lanes) d[j] = sa[j];
    return;
  }
  const uint32_t b = sh & 3u;
  switch (sh >> 2) {  // (uniform over the piece)
    case 0: copy_body<0>(d, sa, b, chunks, t, lanes); break;
    case 1: copy_body<1>(d, sa, b, chunks, t, lanes); break;
    case 2: copy_body<2>(d, sa, b, chunks, t, lanes); break;
    default: copy_body<3>(d, sa, b, chunks, t, lanes); break;
  }
}

// a cut of range r's bytes at x (clamped to [0, len]), moved down onto the destination's 16-byte grid: the pieces on
// both sides of a window's edge then start and end aligned
__device__ inline uint64_t cut_at(int64_t x, uint64_t len, const uint8_t *dst) {
  if (x <= 0) return 0ull;
  if ((uint64_t)x >= len) return len;
  const uint64_t down = (reinterpret_cast<uintptr_t>(dst) + (uint64_t)x) & 15u;
  return (uint64_t)x > down ? (uint64_t)x - down : 0ull;
}

}  // namespace

// Range r occupies the cost interval [S_r, S_r + kBgzfGatherRangeCost + len_r), S_r = r_out_off[r] + r *
// kBgzfGatherRangeCost; its byte q sits at cost S_r + kBgzfGatherRangeCost + q.
__global__ __launch_bounds__(256) void bgzf_gather_kernel(BgzfGatherParams P) {
  const uint64_t C = kBgzfGatherRangeCost;
  const uint64_t A = (uint64_t)blockIdx.x * kBgzfGatherWindow, B = A + kBgzfGatherWindow;
  // the first range whose interval ends above A
  uint32_t lo = 0, hi = P.n_ranges;
  for (int it = 0; it < 33 && lo < hi; ++it) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (P.r_out_off[mid + 1u] + C * (mid + 1ull) <= A) lo = mid + 1u;
    else hi = mid;
  }
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  for (uint32_t r = lo; r < P.n_ranges; ++r) {  // (at most kBgzfGatherWindow / kBgzfGatherRangeCost + 1 rounds)
    const uint64_t at = P.r_out_off[r];
    const uint64_t S = at + C * r;
    if (S >= B) break;
    const uint64_t len = P.r_out_off[r + 1u] - at;
    if (len == 0ull) continue;
    uint8_t *dst = P.out + at;
    const uint64_t q0 = cut_at((int64_t)(A - S - C), len, dst);  // (two's complement: A below S + C is negative)
    const uint64_t q1 = cut_at((int64_t)(B - S - C), len, dst);
    if (q1 <= q0) continue;
    const uint32_t n = (uint32_t)(q1 - q0);  // <= kBgzfGatherWindow + 15: the lower cut was moved down onto the grid
    const uint8_t *src = P.scratch + P.r_src[r] + q0;
    if (n >= 4096u) copy_piece(dst + q0, src, n, threadIdx.x, 256u);
    else if ((r & 3u) == wave) copy_piece(dst + q0, src, n, lane, 64u);
  }
}

}  // namespace flate
