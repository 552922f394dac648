// block_scan.h -- the exclusive prefix sum of the index and layout kernels (stream offsets, member offsets, BGZF
// candidates, range places, the checksum join), device only.  The contract of all three functions:
//   - every thread of the workgroup makes the call, in uniform control flow (the functions use barriers and
//     cross-lane reads), and the workgroup is one-dimensional with exactly 64 * W threads;
//   - wtot is W entries of LDS; every function ends behind a barrier, so wtot is free again when it returns, for
//     the next call or for anything else;
//   - T is a type __shfl_up takes (the project uses uint32_t, uint64_t and int64_t);
//   - the sums are exact integer arithmetic (mod 2^bits of T), hence the same in any grouping: the result does not
//     depend on W or on how a range is cut into chunks.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace flate {

// the sum of x over the lanes 0 .. mine of my wavefront
template <typename T>
__device__ inline T wave_scan_incl(T x) {
  const int lane = threadIdx.x & 63;
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(x, d);
    if (lane >= d) x += o;
  }
  return x;
}

// the sum of v over the threads in front of mine; *sum: over all threads, the same in every thread
template <int W, typename T>
__device__ inline T block_scan_excl(T v, T *wtot, T *sum) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const T x = wave_scan_incl(v);
  if (lane == 63) wtot[wid] = x;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll 4  // (all 16 totals in registers at once cost a kernel with three scans in a row its occupancy)
  for (int w = 0; w < W; ++w) {
    const T t = wtot[w];
    if (w < wid) before += t;
    all += t;
  }
  __syncthreads();  // (everyone has read wtot)
  *sum = all;
  return before + x - v;
}

// One workgroup walks [0, n) in chunks of 64 * W: v = load(i) is element i, store(i, before, v) receives the sum of
// the elements in front of i.  Both are called for i < n only, store(i) behind load(i) in the same thread, in rising
// order of i per thread; n is uniform.  Returns the sum of all elements, to every thread.  (No barrier stands behind
// the last chunk's store calls.)
template <int W, typename T, typename Load, typename Store>
__device__ inline T scan_range(uint32_t n, T *wtot, Load load, Store store) {
  T carry = 0;  // the sum of the chunks in front: a register in every thread
  for (uint32_t base = 0; base < n; base += 64u * W) {
    const uint32_t i = base + threadIdx.x;
    const T v = i < n ? load(i) : T(0);
    T sum;
    const T before = carry + block_scan_excl<W, T>(v, wtot, &sum);
    if (i < n) store(i, before, v);
    carry += sum;
  }
  return carry;
}

}  // namespace flate
