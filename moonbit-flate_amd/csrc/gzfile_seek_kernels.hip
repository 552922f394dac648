// gzfile_seek_kernels.hip -- the seek index of a gzip FILE of any members (flate_hip_gzfile_seek_index: build;
// flate_hip_gzfile_ranges: read), on the index the file's discovery left on the device or the caller handed back
// (flate_kernels.h: GzSeekPointsParams, GzSeekPackParams, GzSeekParams, GzSeekRoundParams; the rule:
// gzfile_seek_rule.h).  Locate, select, layout, compose, resolve and check are one_seek_kernels.hip's, TAIL is
// one_tail_kernel and the gather bgzf_gather_kernel, all unchanged.
//   gzfile_seek_points_kernel   POINTS: one workgroup over the units, the point rule with the member-start mark per
//                               unit, a scan of (point, window) pairs, compaction in stream order, both counts
//   gzfile_seek_pack_kernel     PACK: the round's points as runs of R for bgzf_gather_kernel; a member start is a run
//                               of no bytes, so the window-bearing points fall into their block numbers
//   gzfile_seek_members_kernel  one thread per member: its header ends where the index has its first unit, or an
//                               ordered min into one word ("the same file")
//   gzfile_seek_rel_kernel      one thread per unit: rel(k), TAIL's out_off
//   gzfile_seek_seed_kernel     per unit of a round: its seed and its piece
//   gzfile_seek_load_kernel     the stored windows of the round's points into their R slots, zeros for a member start
// No kernel waits for another workgroup; every loop is bounded by the unit, member or range count, by a header's
// length or by 33 search steps.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "flate_hip.h"
#include "flate_kernels.h"
#include "gzfile_rule.h"
#include "gzfile_seek_rule.h"
#include "window_compose.h"

namespace flate {

__global__ __launch_bounds__(1024) void gzfile_seek_points_kernel(GzSeekPointsParams P) {
  __shared__ int64_t wtot[16];
  // low word: points, high word: points that bear a window
  const int64_t total = scan_range<16, int64_t>(
      P.n, wtot,
      [&](uint32_t k) {
        const bool starts = P.u_start[k] != 0ull;
        if (!gzfile_seek_is_point(P.out_off, k, P.span, starts)) return (int64_t)0;
        return (int64_t)(1ull | (starts ? 0ull : 1ull << 32));
      },
      [&](uint32_t k, int64_t before, int64_t v) {
        if (v) P.point_unit[(uint32_t)((uint64_t)before & 0xffffffffull)] = k;
      });
  if (threadIdx.x == 0) {
    P.counts[0] = (uint32_t)((uint64_t)total & 0xffffffffull);
    P.counts[1] = (uint32_t)((uint64_t)total >> 32);
  }
}

__global__ __launch_bounds__(256) void gzfile_seek_pack_kernel(GzSeekPackParams P) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j > P.np) return;
  const uint32_t base = gzfile_seek_blocks_before(P.member_unit, P.m, P.p_lo, (uint32_t)P.point_unit[P.p_lo]);
  const uint32_t p = P.p_lo + j;
  uint32_t before = P.n_points - P.m;  // behind the last point: every window
  if (p < P.n_points) {
    const uint32_t u = (uint32_t)P.point_unit[p];
    before = gzfile_seek_blocks_before(P.member_unit, P.m, p, u);
    if (j < P.np) P.r_src[j] = (uint64_t)(u - P.u0) * kSeekWindow;  // R[i]: the window in front of unit u0 + i
  }
  P.r_out_off[j] = (uint64_t)(before - base) * kSeekWindow;
}

__global__ __launch_bounds__(256) void gzfile_seek_members_kernel(GzSeekParams G) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= G.m) return;
  // (member_off[j] < in_len: gzfile_seek_index_ok)
  if (gzfile_first_bit(G.in, G.in_len, G.member_off[j]) != G.Q.unit_bit[G.member_unit[j]]) atomicMin(G.bad_member, j);
}

__global__ __launch_bounds__(256) void gzfile_seek_rel_kernel(GzSeekParams G) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k > G.Q.n) return;
  G.rel[k] = k < G.Q.n ? gzfile_seek_rel(G.Q.out_off, G.member_unit, G.m, k) : 0ull;
}

// The list holds, of every segment it enters, the point and the units behind it without a gap (one_seek_seed_kernel).
__global__ __launch_bounds__(256) void gzfile_seek_seed_kernel(GzSeekRoundParams Z) {
  const OneSeekRoundParams &S = Z.S;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= S.count) return;
  const OneSeekParams &Q = S.Q;
  const uint32_t su = Q.sel_unit[S.i0 + i];
  const uint32_t back = su - (uint32_t)Q.point_unit[seek_point_of(Q.point_unit, Q.n_points, su)];  // units behind the point
  S.seed[i] = back <= i ? i - back : 0u;
  S.p_bit_off[i] = Q.unit_bit[su];
  S.p_bit_end[i] = gzfile_seek_runs_to_final(Z.member_unit, Z.m, su) ? ~0ull : Q.unit_bit[su + 1u];
  const uint32_t dict_len = gzfile_seek_dict_len(Z.rel[su]);
  S.p_dict_len[i] = dict_len;
  S.p_dict_at[i] = (uint64_t)(i + 1u) * kWinEntries - dict_len;  // the tail of R[i]; R[i + 1] follows it
}

// One thread per 16 bytes of the round's windows; a slot that is no point's is left alone.  `windows` at any byte
// alignment: byte loads, one 16-byte store.
__global__ __launch_bounds__(256) void gzfile_seek_load_kernel(GzSeekRoundParams Z) {
  const OneSeekRoundParams &S = Z.S;
  const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t per = kWinEntries / 16u;
  const uint32_t i = (uint32_t)(idx / per), j = (uint32_t)(idx % per);
  if (i >= S.count || S.seed[i] != i) return;
  const OneSeekParams &Q = S.Q;
  const uint32_t su = Q.sel_unit[S.i0 + i];
  const uint32_t p = seek_point_of(Q.point_unit, Q.n_points, su);
  if (Q.point_unit[p] != su) return;  // (place 0 of a segment that continues: R[0] is the carried window)
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  const uint32_t mj = bgzf_upper_bound(Z.member_unit, Z.m, su);
  if (Z.member_unit[mj - 1u] != su) {  // (a member start: zeros, nothing of the member in front is ever resolved)
    const uint8_t *src = S.windows + (uint64_t)(p - mj) * kSeekWindow + 16u * j;
    for (uint32_t t = 0; t < 16u; ++t) w[t >> 2] |= (uint32_t)src[t] << (8u * (t & 3u));
  }
  *reinterpret_cast<uint4 *>(S.R + (uint64_t)i * kWinEntries + 16u * j) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace flate
