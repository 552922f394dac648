// seek_pack_kernels.hip -- the PACKED windows of the seek index of ONE long stream (flate_hip_seek_windows_pack /
// _unpack, flate_hip_inflate_one_ranges_packed; the rule: seek_pack_rule.h; flate_kernels.h: SeekPackBlock,
// SeekMarkParams).  MARK + SPARSIFY needs the shared block reader and is seek_pack_mark_kernel.inc, compiled with
// inflate_kernels.hip; the encode and the decode of the blocks are the batch kernels, unchanged.
//   seek_pack_flags_kernel  COMPRESS without SPARSE: one workgroup per block, "has a non-zero byte" and nothing else
//   seek_pack_load_kernel   the read: the unpacked windows of the round's points from the dense stage of the SELECTED
//                           points into their R slots, through the point -> slot table
// No kernel waits for another workgroup; no loop depends on data.
#include <hip/hip_runtime.h>

#include "flate_hip.h"
#include "flate_kernels.h"
#include "seek_pack_rule.h"

namespace flate {

// `windows` at any byte alignment: byte loads, 128 per thread.
__global__ __launch_bounds__(256) void seek_pack_flags_kernel(const uint8_t *windows, uint32_t n_blocks, SeekPackBlock *blk) {
  __shared__ uint32_t any;
  const uint32_t b = blockIdx.x;
  if (b >= n_blocks) return;
  if (threadIdx.x == 0) any = 0u;
  __syncthreads();
  const uint8_t *src = windows + (uint64_t)b * kSeekWindow;
  uint32_t v = 0u;
  for (uint32_t j = threadIdx.x; j < kSeekWindow; j += 256u) v |= src[j];
  if (v) atomicOr(&any, 1u);
  __syncthreads();
  if (threadIdx.x == 0) {
    SeekPackBlock r;
    r.nonzero = any;
    r.kept = kSeekWindow;
    r.status = 0;
    r.pad = 0u;
    blk[b] = r;
  }
}

// one_seek_load_kernel with S.windows the dense stage: slot slot_of_point[p] holds the block of point p (p >= 1; only
// the selected points have a slot, and only they are asked for).  One thread per 16 bytes; the stage is 16-byte aligned.
__global__ __launch_bounds__(256) void seek_pack_load_kernel(OneSeekRoundParams S, const uint32_t *slot_of_point) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t per = kSeekWindow / 16u;
  const uint32_t i = (uint32_t)(idx / per), j = (uint32_t)(idx % per);
  if (i >= S.count || S.seed[i] != i) return;
  const OneSeekParams &Q = S.Q;
  const uint32_t su = Q.sel_unit[S.i0 + i];
  const uint32_t p = seek_point_of(Q.point_unit, Q.n_points, su);
  if (Q.point_unit[p] != su) return;  // (place 0 of a segment that continues: R[0] is the carried window)
  uint4 w = make_uint4(0u, 0u, 0u, 0u);
  if (p > 0u)  // (point 0 is unit 0: in front of the stream, zeros)
    w = *reinterpret_cast<const uint4 *>(S.windows + (uint64_t)slot_of_point[p] * kSeekWindow + 16u * j);
  *reinterpret_cast<uint4 *>(S.R + (uint64_t)i * kSeekWindow + 16u * j) = w;
}

}  // namespace flate
