// one_seek_kernels.hip -- the seek index of ONE long DEFLATE stream (flate_hip_inflate_one_seek_index: build;
// flate_hip_inflate_one_ranges: read), on the index the discovery left on the device or the caller handed back
// (flate_kernels.h: OneSeekPointsParams, OneSeekParams, OneSeekRoundParams; the rule: seek_index_rule.h).
//   one_seek_points_kernel   POINTS: one workgroup over the units, the point rule per unit from two neighbouring
//                            out_off entries, a scan, compaction in stream order
//   one_seek_pack_kernel     PACK: the round's point units as runs of R for bgzf_gather_kernel
//   one_seek_locate_kernel   one thread per range: binary search in out_off, +1 at pstart(first), -1 behind last
//   one_seek_select_kernel   one workgroup over the units: the scan of the differences marks the decoded units, one
//                            scan of (1, size) gives rank and scratch place, compaction in stream order
//   one_seek_layout_kernel   one workgroup over the ranges: the scan of their lengths; a range's bytes are ONE run of
//                            the scratch, every unit from its first to its last being decoded
//   one_seek_seed_kernel     per unit of a round: its seed and its piece
//   one_seek_load_kernel     the stored windows of the round's points into their R slots
//   one_seek_compose_kernel  one step of the SEGMENTED scan of the tail functions
//   one_seek_resolve_kernel  the windows in front of the round's units from their seeds' windows
//   one_seek_check_kernel    a decoded unit is good iff its piece ends with status 0 and fills its slot
// No kernel waits for another workgroup; every loop is bounded by the unit count, the range count or 33 search steps.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "flate_hip.h"
#include "flate_kernels.h"
#include "seek_index_rule.h"
#include "window_compose.h"

namespace flate {

__global__ __launch_bounds__(1024) void one_seek_points_kernel(OneSeekPointsParams P) {
  __shared__ uint32_t wtot[16];
  const uint32_t total = scan_range<16, uint32_t>(
      P.n, wtot, [&](uint32_t k) { return seek_is_point(P.out_off, k, P.span) ? 1u : 0u; },
      [&](uint32_t k, uint32_t before, uint32_t v) {
        if (v) P.point_unit[before] = k;
      });
  if (threadIdx.x == 0) *P.n_points = total;
}

__global__ __launch_bounds__(256) void one_seek_pack_kernel(const uint64_t *point_unit, uint32_t p_lo, uint32_t np,
                                                            uint32_t u0, uint64_t *r_out_off, uint64_t *r_src) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j > np) return;
  r_out_off[j] = (uint64_t)j * kSeekWindow;
  if (j < np) r_src[j] = (point_unit[p_lo + j] - u0) * kSeekWindow;  // R[i]: the window in front of unit u0 + i
}

__global__ __launch_bounds__(256) void one_seek_locate_kernel(OneSeekParams P) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= P.n_ranges) return;
  const SeekLoc L = seek_locate(P.begin[r], P.end[r], P.out_off, P.n, P.point_unit, P.n_points);
  P.r_b[r] = L.b;
  P.r_len[r] = L.e - L.b;
  P.r_first[r] = L.first;
  P.r_last[r] = L.last;
  P.r_seg[r] = L.seg;
  if (L.first != kBgzfNoMember) {  // (seg <= first <= last < n: the array has n + 1 entries)
    atomicAdd(&P.diff[L.seg], 1);
    atomicAdd(&P.diff[L.last + 1u], -1);
  }
}

__global__ __launch_bounds__(1024) void one_seek_select_kernel(OneSeekParams P) {
  __shared__ int64_t wtot[16];
  int64_t cover_c = 0, cnt_c = 0, bytes_c = 0;  // the three sums over the chunks in front
  for (uint32_t base = 0; base < P.n; base += 1024u) {
    const uint32_t k = base + threadIdx.x;
    const bool in = k < P.n;
    const int64_t d = in ? (int64_t)P.diff[k] : 0;
    int64_t dsum, csum, bsum;
    const int64_t cover = cover_c + block_scan_excl<16, int64_t>(d, wtot, &dsum) + d;  // spans [seg, last] that hold k
    const bool sel = in && cover > 0;
    const uint64_t size = sel ? P.out_off[k + 1u] - P.out_off[k] : 0ull;
    const uint64_t rank = (uint64_t)(cnt_c + block_scan_excl<16, int64_t>(sel ? 1 : 0, wtot, &csum));
    const uint64_t at = (uint64_t)(bytes_c + block_scan_excl<16, int64_t>((int64_t)size, wtot, &bsum));
    if (in) {
      P.rank[k] = (uint32_t)rank;
      P.scratch_at[k] = at;
    }
    if (sel) {
      P.sel_unit[rank] = k;
      P.sel_at[rank] = at;
    }
    cover_c += dsum, cnt_c += csum, bytes_c += bsum;
  }
  if (threadIdx.x == 0) {
    P.head->n_sel = (uint32_t)cnt_c;
    P.head->scratch_total = (uint64_t)bytes_c;
    P.head->pad = 0;
    P.sel_at[cnt_c] = (uint64_t)bytes_c;
  }
}

__global__ __launch_bounds__(1024) void one_seek_layout_kernel(OneSeekParams P) {
  __shared__ int64_t wtot[16];
  const uint64_t total = (uint64_t)scan_range<16, int64_t>(
      P.n_ranges, wtot, [&](uint32_t r) { return (int64_t)P.r_len[r]; },
      [&](uint32_t r, int64_t at, int64_t) {
        const uint32_t first = P.r_first[r];
        P.r_out_off[r] = (uint64_t)at;
        if (first != kBgzfNoMember) {
          P.r_src[r] = P.scratch_at[first] + (P.r_b[r] - P.out_off[first]);
          P.r_rank_lo[r] = P.rank[P.r_seg[r]];
          P.r_rank_hi[r] = P.rank[P.r_last[r]] + 1u;
        } else {
          P.r_src[r] = 0ull;
          P.r_rank_lo[r] = 0u;
          P.r_rank_hi[r] = 0u;
        }
      });
  if (threadIdx.x == 0) {
    P.r_out_off[P.n_ranges] = total;
    P.head->out_total = total;
  }
}

// The list holds, of every segment it enters, the point and the units behind it without a gap: a unit that is no
// point has the unit in front of it one place in front of it in the list.
__global__ __launch_bounds__(256) void one_seek_seed_kernel(OneSeekRoundParams S) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= S.count) return;
  const OneSeekParams &Q = S.Q;
  const uint32_t su = Q.sel_unit[S.i0 + i];
  const uint32_t back = su - (uint32_t)Q.point_unit[seek_point_of(Q.point_unit, Q.n_points, su)];  // units behind the point
  S.seed[i] = back <= i ? i - back : 0u;
  S.p_bit_off[i] = Q.unit_bit[su];
  S.p_bit_end[i] = su + 1u < Q.n ? Q.unit_bit[su + 1u] : ~0ull;  // the last unit runs to BFINAL
  const uint64_t at = Q.out_off[su];
  const uint32_t dict_len = at < (uint64_t)kWinEntries ? (uint32_t)at : kWinEntries;
  S.p_dict_len[i] = dict_len;
  S.p_dict_at[i] = (uint64_t)(i + 1u) * kWinEntries - dict_len;  // the tail of R[i]; R[i + 1] follows it
}

// One thread per 16 bytes of the round's windows; a slot that is no point's is left alone.  `windows` at any byte
// alignment: byte loads, one 16-byte store.
__global__ __launch_bounds__(256) void one_seek_load_kernel(OneSeekRoundParams S) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t per = kWinEntries / 16u;
  const uint32_t i = (uint32_t)(idx / per), j = (uint32_t)(idx % per);
  if (i >= S.count || S.seed[i] != i) return;
  const OneSeekParams &Q = S.Q;
  const uint32_t su = Q.sel_unit[S.i0 + i];
  const uint32_t p = seek_point_of(Q.point_unit, Q.n_points, su);
  if (Q.point_unit[p] != su) return;  // (place 0 of a segment that continues: R[0] is the carried window)
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (p > 0u) {  // (point 0 is unit 0: in front of the stream, zeros)
    const uint8_t *src = S.windows + (uint64_t)(p - 1u) * kSeekWindow + 16u * j;
    for (uint32_t t = 0; t < 16u; ++t) w[t >> 2] |= (uint32_t)src[t] << (8u * (t & 3u));
  }
  *reinterpret_cast<uint4 *>(S.R + (uint64_t)i * kWinEntries + 16u * j) = make_uint4(w[0], w[1], w[2], w[3]);
}

// dst[k] = src[k] o src[k - s] where k - s lies at or behind k's seed; one thread per entry.
__global__ __launch_bounds__(256) void one_seek_compose_kernel(const uint16_t *src, uint16_t *dst, const uint32_t *seed,
                                                               uint32_t count, uint32_t s) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t k = idx / kWinEntries;
  if (k >= count) return;
  const uint16_t e = src[idx];
  dst[idx] = (k >= s && k - s >= seed[k]) ? wc_compose(e, src + (k - s) * kWinEntries) : e;
}

// R[k + 1] = F[k] applied to R[seed[k]], F[k] the composition from k's seed up to k.  A seed's slot is slot 0 or a
// point's: neither is written here.
__global__ __launch_bounds__(256) void one_seek_resolve_kernel(const uint16_t *F, uint8_t *R, const uint32_t *seed,
                                                               uint32_t count) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t k = idx / kWinEntries;
  if (k >= count) return;
  if (k + 1u < count && seed[k + 1u] == k + 1u) return;  // the next unit is a point: its slot holds the stored window
  R[kWinEntries + idx] = wc_resolve(F[idx], R + (uint64_t)seed[k] * kWinEntries);
}

__global__ __launch_bounds__(256) void one_seek_check_kernel(OneSeekRoundParams S) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= S.count) return;
  const uint32_t at = S.i0 + i;
  int32_t st = S.d_status[i];
  if (st == 0 && S.d_out_len[i] != S.Q.sel_at[at + 1u] - S.Q.sel_at[at]) st = FLATE_HIP_E_CORRUPT;
  S.u_status[at] = st;
}

}  // namespace flate
