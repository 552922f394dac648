// splice_kernels.hip -- SURVEY.md section 8(f)-3: the streams of a batch as ONE legal DEFLATE
// stream.  The pack kernel writes every stream at its bit position in the spliced stream (and the
// closing block of Writer::close, deflate.mbt:171-176, only once); this file holds the step in
// between: from the per-stream summaries of huff_code_kernel to those bit positions.
//
// The position maps (x -> x + a, x -> align8(x + a) + b), their composition and the groups' rule: splice_rule.h.
#include <hip/hip_runtime.h>

#include "flate_common.h"
#include "flate_kernels.h"
#include "splice_rule.h"
#include "zip_kernels.h"
#include "zip_rule.h"

namespace flate {

// stream_bit[i] = bit position of stream i's first block, stream_bit[n] = end of the last stream;
// *total_bytes = size of the spliced stream including the closing block.  One block of 1024.
__global__ __launch_bounds__(1024) void splice_scan_kernel(SpliceParams P) {
  __shared__ PosMap part[1024];
  const uint32_t t = threadIdx.x;
  const uint64_t n = P.n_streams;
  const uint64_t lo = n * t / 1024, hi = n * (t + 1) / 1024;
  PosMap f = {0, kNoStored};
  for (uint64_t i = lo; i < hi; ++i) f = then(f, PosMap{P.sum[2 * i], P.sum[2 * i + 1]});
  part[t] = f;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {  // inclusive scan of the chunk maps
    PosMap v = part[t];
    if (t >= d) v = then(part[t - d], v);
    __syncthreads();
    part[t] = v;
    __syncthreads();
  }
  uint64_t x = t ? apply(part[t - 1], P.start_bit) : P.start_bit;  // position in front of this thread's chunk
  for (uint64_t i = lo; i < hi; ++i) {
    P.stream_bit[i] = x;
    x = apply(PosMap{P.sum[2 * i], P.sum[2 * i + 1]}, x);
  }
  if (t == 1023) {
    P.stream_bit[n] = x;
    // closing block: 3 bits, padding, LEN, NLEN (not behind a stream that continues in a later call)
    const uint64_t bytes = P.no_close ? (align8(x) >> 3) : (align8(x + 3) >> 3) + 4;
    *P.total_bytes = bytes;
    if (bytes + 3 > P.out_cap) atomicExch(P.status, -2);  // + the rest of the last dword
  }
}

// The pack kernel ORs into the dwords a stream shares with its neighbours (its first and its last
// one) and plainly stores all others, so only those need to be zero beforehand: the dword holding
// bit stream_bit[i] and the one in front of it, for every i, plus the closing block's.
__global__ __launch_bounds__(256) void splice_zero_kernel(SpliceParams P, uint8_t *out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i > P.n_streams || *P.status != 0) return;
  const uint64_t mis = (uint64_t)(reinterpret_cast<uintptr_t>(out) & 3u);
  uint32_t *dst = reinterpret_cast<uint32_t *>(out - mis);
  const uint64_t g = P.stream_bit[i] + 8 * mis;
  if ((g >> 5) == 0) {  // the grid's first dword starts mis bytes in front of out: not ours to write
    for (uint64_t k = mis; k < 4; ++k) out[k - mis] = 0;
  } else {
    dst[g >> 5] = 0;
    if ((g >> 5) == 1) {
      for (uint64_t k = mis; k < 4; ++k) out[k - mis] = 0;
    } else {
      dst[(g >> 5) - 1] = 0;
    }
  }
  if (i == P.n_streams && !P.no_close) {  // closing block: 3 bits, padding, LEN, NLEN -- at most 3 more dwords
    const uint64_t end = (*P.total_bytes + mis) * 8;
    for (uint64_t d = (g >> 5) + 1; d * 32 < end; ++d) dst[d] = 0;
  }
}

// ---- several spliced streams in one output (splice_rule.h: GROUPS; the kernel equals grouped_place) ----

// The same fold, scan and walk over the pieces' maps, with the group's close map behind every piece that is the last
// of its group; the start is the first group's header.  One block of 1024.
__global__ __launch_bounds__(1024) void group_scan_kernel(GroupParams P) {
  __shared__ PosMap part[1024];
  __shared__ uint32_t k0_s;  // ZIP: the first entry whose header offset needs the Zip64 extra
  const uint32_t t = threadIdx.x;
  if (t == 0) k0_s = P.n_groups;
  const uint64_t n = P.n_pieces;
  const uint64_t lo = n * t / 1024, hi = n * (t + 1) / 1024;
  auto map_of = [&](uint64_t i) { return PosMap{P.sum[2 * i], P.sum[2 * i + 1]}; };
  auto last_of = [&](uint64_t i) { return i + 1 == n || P.piece_group[i + 1] != P.piece_group[i]; };
  auto close_of = [&](uint32_t g) {
    return group_close_map(P.trailer_len, g + 1 < P.n_groups ? group_header_len(P.header_len, P.header_len_all, g + 1) : 0u);
  };
  PosMap f = {0, kNoStored};
  for (uint64_t i = lo; i < hi; ++i) {
    f = then(f, map_of(i));
    if (last_of(i)) f = then(f, close_of(P.piece_group[i]));
  }
  part[t] = f;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {  // inclusive scan of the chunk maps
    PosMap v = part[t];
    if (t >= d) v = then(part[t - d], v);
    __syncthreads();
    part[t] = v;
    __syncthreads();
  }
  const uint64_t start = 8ull * group_header_len(P.header_len, P.header_len_all, 0);
  uint64_t x = t ? apply(part[t - 1], start) : start;  // position in front of this thread's chunk
  for (uint64_t i = lo; i < hi; ++i) {
    const uint32_t g = P.piece_group[i];
    P.stream_bit[i] = x;
    if (i == P.group_off[g]) {  // (a multiple of 8: the start, or behind a close map)
      P.payload_off[g] = x >> 3;
      const uint64_t at = (x >> 3) - group_header_len(P.header_len, P.header_len_all, g);
      P.member_off[g] = at;
      if (P.zip_head && zip_central_has_extra(at)) atomicMin(&k0_s, g);
    }
    x = apply(map_of(i), x);
    if (last_of(i)) {
      P.end_bit[g] = x;
      x = apply(close_of(g), x);
    }
  }
  __syncthreads();  // (k0_s is final; payload_off and end_bit of a group may be another thread's)
  if (t == 1023) {
    const uint64_t sum = x >> 3;
    uint64_t total = sum;
    P.stream_bit[n] = x;
    P.member_off[P.n_groups] = sum;
    if (P.zip_head) {  // (zip_scan_kernel's result words)
      ZipWriteHead h;
      h.cd_off = sum;
      h.k0 = k0_s, h.pad = 0;
      h.cd_size = zip_central_place(P.n_groups, P.zip_name_off[P.n_groups] - P.zip_name_off[0], k0_s);
      h.total = sum + h.cd_size + zip_end_len(P.n_groups, sum, h.cd_size);
      *P.zip_head = h;
      total = h.total;
    }
    *P.total_bytes = total;
    if (total + P.slack > P.out_cap) atomicExch(P.status, -2);
  }
  if (!P.bit_idx && !P.zip_head) return;
  for (uint64_t i = lo; i < hi; ++i) {
    const uint32_t g = P.piece_group[i];
    const uint64_t base = 8 * P.payload_off[g];
    if (P.bit_idx) {
      P.bit_idx[i + g] = P.stream_bit[i] - base;
      if (last_of(i)) P.bit_idx[i + 1 + g] = P.end_bit[g] - base;
    }
    // (a ZIP entry's compressed size is a 32-bit field)
    if (P.zip_head && last_of(i) && align8(P.end_bit[g] + 3) + 32 - base >= (1ull << 35))
      atomicExch(P.status, FLATE_HIP_E_TOO_LARGE);
  }
}

// splice_zero_kernel's discipline: the dword holding every piece's first bit and the one in front of it (threads
// 0 .. n_pieces - 1), and from every group's end through its closing block (threads n_pieces .. + n_groups - 1).
// Headers and trailers are written behind the pack kernel with byte stores.
__global__ __launch_bounds__(256) void group_zero_kernel(GroupParams P, uint8_t *out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= (uint64_t)P.n_pieces + P.n_groups || *P.status != 0) return;
  const bool group = i >= P.n_pieces;
  const uint64_t bit = group ? P.end_bit[i - P.n_pieces] : P.stream_bit[i];
  const uint64_t mis = (uint64_t)(reinterpret_cast<uintptr_t>(out) & 3u);
  uint32_t *dst = reinterpret_cast<uint32_t *>(out - mis);
  const uint64_t g = bit + 8 * mis;
  if ((g >> 5) == 0) {  // the grid's first dword starts mis bytes in front of out: not ours to write
    for (uint64_t k = mis; k < 4; ++k) out[k - mis] = 0;
  } else {
    dst[g >> 5] = 0;
    if ((g >> 5) == 1) {
      for (uint64_t k = mis; k < 4; ++k) out[k - mis] = 0;
    } else {
      dst[(g >> 5) - 1] = 0;
    }
  }
  if (group) {  // closing block: 3 bits, padding, LEN, NLEN -- at most 2 more dwords
    const uint64_t end = align8(g + 3) + 32;
    for (uint64_t d = (g >> 5) + 1; d * 32 < end; ++d) dst[d] = 0;
  }
}

}  // namespace flate
